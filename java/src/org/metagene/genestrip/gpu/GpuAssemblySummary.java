/*
 * The picks of a Genbank assembly summary per tree node (gs_asmsum, include/gsgpu.h) as a handle with close(): made by
 * gs_host_asmsum_files from the summary file, the cap of FastaFilesFromGenbankGoal applied, fetched once.
 * SOURCE ONLY (no JDK in the build container).
 */
package org.metagene.genestrip.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.nio.charset.StandardCharsets;

public final class GpuAssemblySummary implements AutoCloseable {
	private long handle;
	private final int picked;
	private final long counted;
	private int[] nodes;
	private byte[] quality;
	private byte[] isRef;
	private long[] strOff;
	private byte[] pool;

	private GpuAssemblySummary(long handle, int picked, long counted) {
		this.handle = handle;
		this.picked = picked;
		this.counted = counted;
	}

	/** filter: nNodes bytes (1: a node of the taxfromgenbank set) or null for every node; qualityMask: bit q allows the
	 *  AssemblyQuality of ordinal q, -1 is the reference's null list */
	public static GpuAssemblySummary fromFiles(String[] paths, int device, ByteBuffer knownTaxids, int nNodes, ByteBuffer filter,
			int qualityMask, boolean referenceOnly, boolean useSpeciesTaxid, int maxPerNode) {
		long[] totals = new long[7];
		long h = GsGpuNative.hostAsmsumFiles(paths, device, knownTaxids, knownTaxids.capacity() / 4, nNodes, filter,
				filter == null ? 0 : filter.capacity(), qualityMask, referenceOnly, useSpeciesTaxid, 0, maxPerNode, totals);
		return new GpuAssemblySummary(h, (int) totals[3], totals[1]);
	}

	/** entries behind the cap */
	public int picked() {
		return picked;
	}

	/** records of 20 fields and more: totalEntries[0] of AssemblySummaryReader.getRelevantEntries */
	public long counted() {
		return counted;
	}

	private void fetch() {
		if (nodes != null) {
			return;
		}
		int m = picked;
		ByteBuffer n = GpuTaxTree.ints(m);
		ByteBuffer q = ByteBuffer.allocateDirect(Math.max(m, 1));
		ByteBuffer r = ByteBuffer.allocateDirect(Math.max(m, 1));
		ByteBuffer off = ByteBuffer.allocateDirect(8 * (3 * m + 1)).order(ByteOrder.nativeOrder());
		GsGpuNative.asmsumFetch(handle, n, m, q, m, r, m, null, 0, off, 3 * m + 1, null, 0);
		long bytes = off.getLong(8 * 3 * m);
		ByteBuffer p = ByteBuffer.allocateDirect((int) Math.max(bytes, 1));
		GsGpuNative.asmsumFetch(handle, null, 0, null, 0, null, 0, null, 0, null, 0, p, bytes);
		nodes = new int[m];
		n.asIntBuffer().get(nodes);
		quality = new byte[m];
		q.get(quality);
		isRef = new byte[m];
		r.get(isRef);
		strOff = new long[3 * m + 1];
		off.asLongBuffer().get(strOff);
		pool = new byte[(int) bytes];
		p.get(pool);
	}

	/** node of pick i; the picks come grouped by ascending node, inside a node in the reference's list order */
	public int node(int i) {
		fetch();
		return nodes[i];
	}

	/** ordinal of the AssemblyQuality of pick i */
	public int quality(int i) {
		fetch();
		return quality[i];
	}

	public boolean isReference(int i) {
		fetch();
		return isRef[i] != 0;
	}

	/** which = 0: tax id, 1: species tax id, 2: ftp path of pick i, as the file's bytes */
	public String string(int i, int which) {
		fetch();
		int from = (int) strOff[3 * i + which];
		return new String(pool, from, (int) strOff[3 * i + which + 1] - from, StandardCharsets.UTF_8);
	}

	@Override
	public void close() {
		if (handle != 0L) {
			GsGpuNative.asmsumDestroy(handle);
			handle = 0L;
		}
	}
}
