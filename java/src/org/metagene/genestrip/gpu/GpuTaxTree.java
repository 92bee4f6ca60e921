/*
 * The tree of an NCBI taxonomy dump on the device (gs_taxtree, include/gsgpu.h) as a handle with close().  A node is its index in
 * the ascending array of distinct tax ids; taxIds() is the knownTaxids every other handle of the database chain takes.
 * SOURCE ONLY (no JDK in the build container); tools/check_java_glue.py checks the reference members used under java/src.
 */
package org.metagene.genestrip.gpu;

import java.io.File;
import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.util.Arrays;

public final class GpuTaxTree implements AutoCloseable {
	private long handle;
	private final int nNodes;
	private final int nReached;
	private int[] taxIds;

	private GpuTaxTree(long handle, int nNodes, int nReached) {
		this.handle = handle;
		this.nNodes = nNodes;
		this.nReached = nReached;
	}

	/** gs_host_taxtree_files over dir/nodes.dmp and, if withNames, dir/names.dmp: what TaxTree(File, boolean) reads */
	public static GpuTaxTree load(int device, File dir, boolean withNames) {
		long[] report = new long[8];
		long h = GsGpuNative.hostTaxtreeFiles(device, new File(dir, "nodes.dmp").getPath(),
				withNames ? new File(dir, "names.dmp").getPath() : null, report);
		return new GpuTaxTree(h, (int) report[4], (int) report[5]);
	}

	public long handle() {
		return handle;
	}

	public int size() {
		return nNodes;
	}

	/** nodes the root reaches: the room gs_taxtree_small's outputs need */
	public int reached() {
		return nReached;
	}

	/** the ascending distinct tax ids; index = node */
	public int[] taxIds() {
		if (taxIds == null) {
			ByteBuffer ids = ints(nNodes);
			GsGpuNative.taxtreeFetch(handle, ids, nNodes, null, 0, null, 0, null, 0, null, 0, null, 0);
			int[] res = new int[nNodes];
			ids.asIntBuffer().get(res);
			taxIds = res;
		}
		return taxIds;
	}

	/** taxIds() as the direct buffer the natives take */
	public ByteBuffer taxIdBuffer() {
		ByteBuffer ids = ints(nNodes);
		ids.asIntBuffer().put(taxIds());
		return ids;
	}

	/** the node of a tax id string as the reference keys it, or -1: what is no number of 1-9 digits names no node here */
	public int nodeOf(String taxId) {
		if (taxId == null || taxId.isEmpty() || taxId.length() > 9 || taxId.charAt(0) == '0') {
			return -1;
		}
		int v = 0;
		for (int i = 0; i < taxId.length(); i++) {
			char ch = taxId.charAt(i);
			if (ch < '0' || ch > '9') {
				return -1;
			}
			v = 10 * v + (ch - '0');
		}
		int pos = Arrays.binarySearch(taxIds(), v);
		return pos >= 0 ? pos : -1;
	}

	/** gs_taxtree_regions_below: regions = nodes x int32 (GpuAccessionMap.regions()); returns the selected nodes below the limit */
	public int[] regionsBelow(ByteBuffer regions, int[] selected, int limit, int checkRankOrdinal) {
		ByteBuffer below = ints(selected.length);
		long n = GsGpuNative.taxtreeRegionsBelow(handle, regions, regions.capacity() / 4, selected, selected.length, limit, checkRankOrdinal,
				null, 0, below, selected.length);
		int[] res = new int[(int) n];
		below.asIntBuffer().get(res);
		return res;
	}

	static ByteBuffer ints(int n) {
		return ByteBuffer.allocateDirect(4 * Math.max(n, 1)).order(ByteOrder.nativeOrder());
	}

	@Override
	public void close() {
		if (handle != 0L) {
			GsGpuNative.taxtreeDestroy(handle);
			handle = 0L;
		}
	}
}
