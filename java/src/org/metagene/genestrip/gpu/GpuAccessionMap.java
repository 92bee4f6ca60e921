/*
 * The accession map of the RefSeq catalog on the device (gs_accmap, include/gsgpu.h) as a handle with close(): made by
 * gs_host_accmap_files from the catalog file(s), fetched once to fill an AccessionMapImpl, or handed to
 * GsGpuNative.hostGenomeFilesInto, which looks the header lines of the genome files up where the device scan left them.
 * SOURCE ONLY (no JDK in the build container).
 */
package org.metagene.genestrip.gpu;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;

public final class GpuAccessionMap implements AutoCloseable {
	/** bytes of a key slot: the accession's length, its bytes, zeros */
	public static final int SLOT = 32;

	private long handle;
	private final int nNodes;
	private final long entries;
	private final long passing;

	private GpuAccessionMap(long handle, int nNodes, long entries, long passing) {
		this.handle = handle;
		this.nNodes = nNodes;
		this.entries = entries;
		this.passing = passing;
	}

	/** the accmapsize number: gs_host_accmap_files with count_only; needs no tree */
	public static long countPassing(String[] catalogs, int device, boolean dna, boolean rna, boolean mrna, String[] categories, String[] statuses) {
		long[] totals = new long[5];
		GsGpuNative.hostAccmapFiles(catalogs, device, dna, rna, mrna, categories, statuses, null, 0, 0, 0, true, totals);
		return totals[1];
	}

	/** the accmap goal: knownTaxids = the tree's ascending tax ids (GpuTaxTree.taxIdBuffer()) */
	public static GpuAccessionMap fromCatalogs(String[] catalogs, int device, boolean dna, boolean rna, boolean mrna, String[] categories,
			String[] statuses, ByteBuffer knownTaxids, int nNodes, long reserveEntries) {
		long[] totals = new long[5];
		long h = GsGpuNative.hostAccmapFiles(catalogs, device, dna, rna, mrna, categories, statuses, knownTaxids, knownTaxids.capacity() / 4,
				nNodes, reserveEntries, false, totals);
		return new GpuAccessionMap(h, nNodes, totals[2], totals[1]);
	}

	public long handle() {
		return handle;
	}

	public long entries() {
		return entries;
	}

	public long passing() {
		return passing;
	}

	/** the sorted key slots, entries() x SLOT bytes */
	public ByteBuffer keys() {
		ByteBuffer keys = ByteBuffer.allocateDirect((int) Math.max(SLOT * entries, 1));
		GsGpuNative.accmapFetch(handle, keys, SLOT * entries, null, 0, null, 0);
		return keys;
	}

	/** the node of every entry, entries() x int32 */
	public ByteBuffer nodes() {
		ByteBuffer nodes = ByteBuffer.allocateDirect((int) Math.max(4 * entries, 4)).order(ByteOrder.nativeOrder());
		GsGpuNative.accmapFetch(handle, null, 0, nodes, entries, null, 0);
		return nodes;
	}

	/** entries per node itself (TaxIdNode.incRefSeqRegions before it walks up), nNodes x int32 */
	public ByteBuffer regions() {
		ByteBuffer regions = GpuTaxTree.ints(nNodes);
		GsGpuNative.accmapFetch(handle, null, 0, null, 0, regions, nNodes);
		return regions;
	}

	@Override
	public void close() {
		if (handle != 0L) {
			GsGpuNative.accmapDestroy(handle);
			handle = 0L;
		}
	}
}
