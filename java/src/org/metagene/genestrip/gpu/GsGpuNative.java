/*
 * Reference-side binding of include/gsgpu.h.  SOURCE ONLY: the build container has no JDK (no javac, no jni.h),
 * so this file and java/jni/gsgpu_jni.c are not compiled here; tools/check_java_glue.py checks every use of a reference
 * member in java/src against the reference's sources instead (see INTEGRATION.md).
 *
 * One static native method per C entry point.  Handles travel as long; batches as direct ByteBuffers
 * (address + length are taken with GetDirectBufferAddress, no copies on the Java side).
 * A non-zero status from the C ABI is turned into a RuntimeException carrying gs_last_error().
 */
package org.metagene.genestrip.gpu;

import java.nio.ByteBuffer;

public final class GsGpuNative {
	static {
		System.loadLibrary("gsgpu_jni"); // links against libgsgpu.so
	}

	private GsGpuNative() {
	}

	/** gs_device_count */
	public static native int deviceCount();

	/** gs_db_create: kmers = n_entries x int64 in KMerStore.visit order (reference encoding), valueIdx = n_entries x
	 *  int32, parentVi = n_values x int32 (-1 root, -2 no node) or null.  Returns the gs_db handle. */
	public static native long dbCreate(int device, int k, long nEntries, ByteBuffer kmers, ByteBuffer valueIdx,
			int nValues, ByteBuffer parentVi);

	/** gs_db_create_striped: ONE store whose record table is split over several GPUs (a store that does not fit one of
	 *  them).  devicesThenHandles holds the device of every stripe on entry and the gs_db handle of every stripe on return;
	 *  begin one run per handle (matchBegin), deal the reads to them, matchMerge, matchFinish on any. */
	public static native void dbCreateStriped(long[] devicesThenHandles, int k, long nEntries, ByteBuffer kmers,
			ByteBuffer valueIdx, int nValues, ByteBuffer parentVi);

	/** gs_dbbuild_begin: DB construction on the device (FillDBGoal + DBGoal); parentVi as for dbCreate, exactly one root */
	public static native long dbBuildBegin(int device, int k, int nValues, ByteBuffer parentVi, boolean lowerCaseBases,
			int maxDust, int stepSize);

	/** gs_dbbuild_add: nRegions regions (bases without headers and line ends, offsets = nRegions + 1 x int64 from 0,
	 *  nodeVi = nRegions x int32, all direct buffers in native order); update = a DBGoal region */
	public static native void dbBuildAdd(long builder, ByteBuffer bases, ByteBuffer offsets, ByteBuffer nodeVi, long nRegions,
			boolean update);

	/** gs_dbbuild_finish: sort + LCA fold; returns the number of stored k-mers */
	public static native long dbBuildFinish(long builder);

	/** gs_dbbuild_fetch: kmers (n x int64 ascending, the reference's encoding) and value indices (n x int32) */
	public static native void dbBuildFetch(long builder, ByteBuffer kmers, ByteBuffer valueIdx);

	/** gs_dbbuild_to_db: the store over the built arrays, laid out on the device (returns a gs_db handle as dbCreate does) */
	public static native long dbBuildToDb(long builder);

	public static native void dbBuildDestroy(long builder);

	/** gs_dbquality_begin: store quality against its source genomes (DBQualityCountsGoal.handleStore) on the store's device;
	 * k, the values and the tree are the store's, the other arguments as for dbBuildBegin */
	public static native long dbQualityBegin(long db, boolean lowerCaseBases, int maxDust, int stepSize);

	/** gs_dbquality_set_range: only the canonical k-mers in [lo, hi); after dbQualityFinish it starts the next pass */
	public static native void dbQualitySetRange(long quality, long lo, long hi);

	/** gs_dbquality_add: regions as for dbBuildAdd; leafVi = nRegions x int32, the value index of each region's leaf node
	 * (AbstractUpdateFastaReader.updateLeafNode), negative: the region counts nothing.  Direct buffers in native order. */
	public static void dbQualityAdd(long quality, ByteBuffer bases, ByteBuffer offsets, ByteBuffer leafVi, long nRegions) {
		dbQualityAdd0(quality, bases, bases.capacity(), offsets, offsets.capacity(), leafVi, leafVi.capacity(), nRegions);
	}

	/** gs_dbquality_finish: counts = nValues x 3 x int64 (tp, tp+fp, tp+fn per value index), present = nValues bytes (1: the value
	 * has an entry in DBQualityCountsGoal's map) */
	public static void dbQualityFinish(long quality, int nValues, ByteBuffer counts, ByteBuffer present) {
		dbQualityFinish0(quality, nValues, counts, counts.capacity(), present, present.capacity());
	}

	public static native void dbQualityDestroy(long quality);

	private static native void dbQualityAdd0(long quality, ByteBuffer bases, long basesCap, ByteBuffer offsets, long offsetsCap,
			ByteBuffer leafVi, long leafViCap, long nRegions);

	private static native void dbQualityFinish0(long quality, int nValues, ByteBuffer counts, long countsCap, ByteBuffer present,
			long presentCap);

	/** gs_dbupdate_begin: a finished store (kmers = nKmers x int64 ascending, valueIdx = nKmers x int32, as dbBuildFetch returns
	 * them or as a KMerSortedArray holds them) goes to the device to be updated in batches (DBGoal.MyFastaReader as a stream);
	 * the other arguments as for dbBuildBegin.  Direct buffers in native order; a buffer shorter than its element count:
	 * IllegalArgumentException. */
	public static long dbUpdateBegin(int device, int k, int nValues, ByteBuffer parentVi, boolean lowerCaseBases, int maxDust,
			int stepSize, ByteBuffer kmers, ByteBuffer valueIdx, long nKmers) {
		return dbUpdateBegin0(device, k, nValues, parentVi, parentVi.capacity(), lowerCaseBases, maxDust, stepSize, kmers,
				kmers == null ? 0 : kmers.capacity(), valueIdx, valueIdx == null ? 0 : valueIdx.capacity(), nKmers);
	}

	/** gs_dbupdate_begin_db: the k-mers of a live store (dbCreate, dbLoad, dbBuildToDb); k, the values and the tree are the store's */
	public static native long dbUpdateBeginDb(long db, boolean lowerCaseBases, int maxDust, int stepSize);

	/** gs_dbupdate_add: regions as for dbBuildAdd(..., update = true): every stored k-mer of a region gets the LCA of its value and
	 * the region's node.  Batches may come in any order and in any number. */
	public static void dbUpdateAdd(long updater, ByteBuffer bases, ByteBuffer offsets, ByteBuffer nodeVi, long nRegions) {
		dbUpdateAdd0(updater, bases, bases.capacity(), offsets, offsets.capacity(), nodeVi, nodeVi.capacity(), nRegions);
	}

	/** gs_dbupdate_finish: returns the number of stored k-mers whose value differs from the value at dbUpdateBegin */
	public static native long dbUpdateFinish(long updater);

	/** the number of k-mers of the store being updated: what dbUpdateFetch writes */
	public static native long dbUpdateSize(long updater);

	/** gs_dbupdate_fetch: kmers (dbUpdateSize x int64 ascending) and value indices (dbUpdateSize x int32) after dbUpdateFinish */
	public static void dbUpdateFetch(long updater, ByteBuffer kmers, ByteBuffer valueIdx) {
		dbUpdateFetch0(updater, kmers, kmers.capacity(), valueIdx, valueIdx.capacity());
	}

	/** gs_dbupdate_to_db: the store over the updated arrays, laid out on the device (returns a gs_db handle as dbCreate does) */
	public static native long dbUpdateToDb(long updater);

	public static native void dbUpdateDestroy(long updater);

	private static native long dbUpdateBegin0(int device, int k, int nValues, ByteBuffer parentVi, long parentViCap,
			boolean lowerCaseBases, int maxDust, int stepSize, ByteBuffer kmers, long kmersCap, ByteBuffer valueIdx,
			long valueIdxCap, long nKmers);

	private static native void dbUpdateAdd0(long updater, ByteBuffer bases, long basesCap, ByteBuffer offsets, long offsetsCap,
			ByteBuffer nodeVi, long nodeViCap, long nRegions);

	private static native void dbUpdateFetch0(long updater, ByteBuffer kmers, long kmersCap, ByteBuffer valueIdx, long valueIdxCap);

	/** gs_dbsize_begin: a collection sized before it is built (FillSizeGoal + FillBloomFilterGoal on the device): nValues tags,
	 * no tree; histBits 1 .. 12; radixBits 0 or GSConfigKey.RADIX_STORE_BITS; keepKeys false: counts only (no dbSizeDistinct) */
	public static native long dbSizeBegin(int device, int k, int nValues, boolean lowerCaseBases, int maxDust, int stepSize, int histBits,
			int radixBits, boolean keepKeys);

	/** gs_dbsize_set_range: only the canonical k-mers in [lo, hi) are retained; after dbSizeCounts / dbSizeDistinct it starts the
	 * next pass with every counter at zero */
	public static native void dbSizeSetRange(long sizer, long lo, long hi);

	/** gs_dbsize_add: regions as for dbBuildAdd; tagVi = nRegions x int32 in [0, nValues).  Direct buffers in native order; a
	 * buffer shorter than its element count: IllegalArgumentException. */
	public static void dbSizeAdd(long sizer, ByteBuffer bases, ByteBuffer offsets, ByteBuffer tagVi, long nRegions) {
		dbSizeAdd0(sizer, bases, bases.capacity(), offsets, offsets.capacity(), tagVi, tagVi.capacity(), nRegions);
	}

	/** gs_dbsize_counts: totals = 3 x int64 (k-mers with duplicates, dropped by the dust gate, included: what FillSizeGoal sets),
	 * perValue = nValues x int64, hist = 2^min(histBits, 2k) x int64, with nValues and histBits as given to dbSizeBegin */
	public static void dbSizeCounts(long sizer, ByteBuffer totals, ByteBuffer perValue, ByteBuffer hist) {
		dbSizeCounts0(sizer, totals, totals.capacity(), perValue, perValue.capacity(), hist, hist.capacity());
	}

	/** gs_dbsize_distinct: returns the number of distinct retained k-mers; bucketSizes = 2^radixBits x int64 (null with
	 * radixBits 0): FillBloomFilterGoal's DBSize(size, bucketSizes), exact */
	public static long dbSizeDistinct(long sizer, ByteBuffer bucketSizes) {
		return dbSizeDistinct0(sizer, bucketSizes, bucketSizes == null ? 0 : bucketSizes.capacity());
	}

	/** gs_dbsize_plan: ranges of the canonical k-mer that hold at most maxPairs k-mers each, from a dbSizeCounts histogram;
	 * bounds = room for cap + 1 x int64, range i is [bounds[i], bounds[i + 1]); returns the number of ranges.  Needs no device. */
	public static int dbSizePlan(ByteBuffer hist, int histBits, int k, long maxPairs, ByteBuffer bounds, int cap) {
		return dbSizePlan0(hist, hist.capacity(), histBits, k, maxPairs, bounds, bounds.capacity(), cap);
	}

	public static native void dbSizeDestroy(long sizer);

	private static native void dbSizeAdd0(long sizer, ByteBuffer bases, long basesCap, ByteBuffer offsets, long offsetsCap,
			ByteBuffer tagVi, long tagViCap, long nRegions);

	private static native void dbSizeCounts0(long sizer, ByteBuffer totals, long totalsCap, ByteBuffer perValue, long perValueCap,
			ByteBuffer hist, long histCap);

	private static native long dbSizeDistinct0(long sizer, ByteBuffer bucketSizes, long bucketSizesCap);

	private static native int dbSizePlan0(ByteBuffer hist, long histCap, int histBits, int k, long maxPairs, ByteBuffer bounds,
			long boundsCap, int cap);

	/** gs_db_save / gs_db_load: the native image of the device store */
	public static native void dbSave(long db, String path);

	public static native long dbLoad(int device, String path);

	public static native void dbDestroy(long db);

	/** gs_match_begin */
	public static native long matchBegin(long db, boolean classify, boolean countUnique, int maxPaths, int threshold,
			double maxReadTaxErr, double maxReadClassErr, int maxKmerResCounts);

	/** gs_match_submit with GS_MEM_HOST: seq = concatenated read bytes, offsets = (nReads+1) x uint64,
	 *  classVi = nReads x int32 (or null), flags = nReads x uint8 (or null). */
	public static native void matchSubmit(long run, ByteBuffer seq, ByteBuffer offsets, long nReads, long firstReadNo,
			ByteBuffer classVi, ByteBuffer flags);

	/** gs_match_submit_async: queues a host batch (best in buffers from pinnedAlloc) and returns its ticket; the buffers
	 *  belong to the library until matchWait(ticket).  Two batches can be under way: the copy of one runs under the
	 *  kernel of the other. */
	public static native long matchSubmitAsync(long run, ByteBuffer seq, ByteBuffer offsets, long nReads, long firstReadNo,
			ByteBuffer classVi, ByteBuffer flags);

	public static native void matchWait(long run, long ticket);

	/** gs_match_submit_text with GS_MEM_HOST: text = a direct buffer holding whole four-line FASTQ records, nLines =
	 *  number of '\n' in it (a multiple of 4).  Returns the ticket; the buffer may be refilled after matchTextWaitCopy. */
	public static native long matchSubmitText(long run, ByteBuffer text, long nBytes, long nLines, long firstReadNo);

	public static native void matchTextWaitCopy(long run, long ticket);

	/** gs_match_text_status: out[0] = ticket of the first refused chunk or -1, out[1] = first bad record or -1,
	 *  out[2..4] = reads, k-mers, bases of the accepted chunks. */
	public static native void matchTextStatus(long run, long[] out);

	public static native void matchTextClearError(long run);

	/** gs_pinned_alloc as a direct buffer (native byte order is up to the caller): the place to stage batches and text
	 *  chunks -- copies from page-locked memory run at the full host-to-device rate.  Free it with pinnedFree, never
	 *  let it be garbage collected while a submit may still read it. */
	public static native ByteBuffer pinnedAlloc(long bytes);

	public static native void pinnedFree(ByteBuffer buf);

	/** gs_match_segments with GS_MEM_HOST: the Kraken-style runs of the reads of a batch; segOff = (nReads+1) x uint64 */
	public static native void matchSegments(long run, ByteBuffer seq, ByteBuffer offsets, long nReads, ByteBuffer segOff);

	/** gs_match_segments_fetch: codes / starts = n_segments x int32 (n_segments = segOff[nReads]) */
	public static native void matchSegmentsFetch(long run, ByteBuffer codes, ByteBuffer starts);

	/** gs_match_max_contig_reads: readNo = n_values x int64 */
	public static native void matchMaxContigReads(long run, ByteBuffer readNo);

	/** gs_match_max_counts: out = (n_values + 1) x maxKmerResCounts int16 */
	public static native void matchMaxCounts(long run, ByteBuffer out);

	/** gs_match_merge: the runs of this process (one per GPU) into a global state held by each */
	public static native void matchMerge(long[] runs);

	/** gs_match_finish: table = n_values x GS_N_COLS int64, dtable = n_values x GS_N_DCOLS double. */
	public static native void matchFinish(long run, ByteBuffer table, ByteBuffer dtable);

	public static native void matchReset(long run);

	public static native void matchDestroy(long run);

	/** gs_bloom_create */
	public static native long bloomCreate(int device, int kind, long bits, int nHashes, long[] hashFactors,
			ByteBuffer words, long nWords);

	/** gs_bloom_build: the XOR index filter of BloomIndexGoal built on the device from nKmers k-mers (direct buffer, int64 in
	 *  native order), sized for expectedInsertions at fpp; returns the gs_bloom handle (as bloomCreate does) */
	public static native long bloomBuild(int device, ByteBuffer kmers, long nKmers, long expectedInsertions, double fpp);

	public static native void bloomDestroy(long bloom);

	/** gs_filter_submit with GS_MEM_HOST: accept = nReads x uint8 */
	public static native void filterSubmit(long bloom, int k, int minPosCount, double positiveRatio, ByteBuffer seq,
			ByteBuffer offsets, long nReads, ByteBuffer accept);

	/**
	 * gs_host_match_files (include/gshost.h): one runMatcher over LOCAL FILES below the JVM -- file, gunzip (on the device), record
	 * scan, kernels, per-read outputs (gathered and gzip-compressed on the device) -- with a run of its own.  paths: the FASTQ /
	 * FASTA files in order; filteredPath / krakenOutPath: null = off, a name ending in .gz / .gzip is written gzip (BGZF members);
	 * taxids: tax id per value index (needed for Kraken-style lines, else null); table / dtable as matchFinish; maxContigDesc: null,
	 * or nValues x descStride bytes that receive CountsPerTaxid.maxContigDescriptor per value index (NUL-terminated);
	 * totals[4] = totalReads, totalKMers, totalBPs, reads written to filteredPath.
	 */
	public static native void hostMatchFiles(long db, boolean classify, boolean countUnique, int maxPaths, int threshold,
			double maxReadTaxErr, double maxReadClassErr, int maxKmerResCounts, String[] paths, String filteredPath,
			String krakenOutPath, boolean writeAll, String[] taxids, boolean withProbs, ByteBuffer table, ByteBuffer dtable,
			ByteBuffer maxContigDesc, int descStride, long[] totals);

	/** gs_host_match_run: the same into the matcher's own run -- matchReset before, matchFinish (and matchMaxCounts) after */
	public static native void hostMatchRun(long run, long db, String[] paths, String filteredPath, String krakenOutPath,
			boolean writeAll, String[] taxids, boolean withProbs, ByteBuffer maxContigDesc, int descStride, long[] totals);

	/** gs_host_match_into: some of a sample's files into a run that is merged with the runs of other GPUs (matchMerge) before
	 *  matchFinish; fileIndex[i] = position of paths[i] in the sample's file order, readsOfFile[i] receives its read count */
	public static native void hostMatchInto(long run, long db, String[] paths, int[] fileIndex, long[] readsOfFile, long[] totals);

	/** gs_host_filter_files: one runFilter over local files; filteredPath / restPath: null = off, .gz = gzip; totals as above
	 *  (totals[3] = accepted reads) */
	public static native void hostFilterFiles(long bloom, int k, int minPosCount, double positiveRatio, String[] paths,
			String filteredPath, String restPath, boolean withProbs, long[] totals);

	/** gs_host_extract_files: the extract goal over local files (FASTQ or FASTA by suffix; plain, gzip, BGZF): every read whose
	 *  descriptor behind its first character starts with key goes to outPath (.gz = gzip) with its qualities; totals as above
	 *  (totals[3] = reads written) */
	public static native void hostExtractFiles(int device, String key, int k, String[] paths, String outPath, long[] totals);

	/** gs_host_fasta2fastq: the fasta2fastq goal over local files: all of them into ONE four-line FASTQ file with '~' qualities
	 *  (.gz = gzip); returns the records written */
	public static native long hostFasta2Fastq(int device, String[] paths, String outPath);

	/** gs_host_last_error: the message of the last failure inside the host layer on this thread */
	public static native String hostLastError();

	/** gs_host_control_create without a callback: the handle of a progress / cancel control.  A file-level call (hostMatchFiles,
	 *  hostMatchRun, hostMatchInto, hostFilterFiles, hostExtractFiles, hostFasta2Fastq) made by the thread that attached it publishes
	 *  its records there and stops when it is cancelled: the call then throws a RuntimeException whose message starts with
	 *  "cancelled" (its totals are filled), and the state and outputs cover exactly the reads of the last snapshot. */
	public static native long hostControlCreate();

	public static native void hostControlDestroy(long control);

	/** any thread */
	public static native void hostControlCancel(long control);

	/** the calling thread's file-level calls use the control until hostControlAttach(0) */
	public static native void hostControlAttach(long control);

	/** any thread; out[SNAPSHOT_LEN]: the latest record -- indices S_* -- and the cancel flag */
	public static native void hostControlSnapshot(long control, long[] out);

	public static final int S_FILE = 0, S_N_FILES = 1, S_FILE_DONE = 2, S_FILES_DONE = 3, S_FILE_BYTES_DONE = 4, S_FILE_BYTES_TOTAL = 5,
			S_FILE_READS = 6, S_TOTAL_BYTES_DONE = 7, S_TOTAL_BYTES_TOTAL = 8, S_TOTAL_READS = 9, S_FILE_MS = 10, S_TOTAL_MS = 11,
			S_CANCELLED = 12, SNAPSHOT_LEN = 13;

	/** true for the exception of a call that was stopped through its control */
	public static boolean isCancelled(RuntimeException e) {
		return e.getMessage() != null && e.getMessage().startsWith("cancelled");
	}

	/** gs_host_release_pools: page-locked blocks and device decoders the host layer keeps from call to call go back to the system */
	public static native void hostReleasePools();

	// ---- the database-construction chain: gs_genomes_*, gs_accmap_*, gs_asmsum_*, gs_taxtree_* and their file-level calls.
	// Arguments in C order.  Every direct buffer (native order) is followed by its capacity in ELEMENTS of its type -- for an int32
	// array buffer.capacity() / 4, for text, keys32 and pools the bytes -- and a call that needs more throws
	// IllegalArgumentException before the library is entered.  The handles of these four families are good for the natives of
	// their family, for accmapLookupGenomes and for hostGenomeFilesInto.  The file-level calls (host*) run under the control the
	// calling thread attached (hostControlAttach) and throw the "cancelled" RuntimeException when it stops them.

	/** gs_genomes_create */
	public static native long genomesCreate(int device);

	/** gs_genomes_scan with GS_MEM_HOST; out[4] = n_records, consumed_bytes, header_bytes, max_line_bytes */
	public static native void genomesScan(long genomes, ByteBuffer text, long textCap, long nBytes, boolean last, long[] out);

	/** gs_genomes_headers: headers = header_bytes, headerOff = n_records + 1 x int64 */
	public static native void genomesHeaders(long genomes, ByteBuffer headers, long headersCap, ByteBuffer headerOff, long headerOffCap);

	/** gs_genomes_gather: keep = n_records bytes or null (every record); out[2] = n_regions, n_bases */
	public static native void genomesGather(long genomes, ByteBuffer keep, long keepCap, long[] out);

	/** gs_genomes_regions: out[2] = the DEVICE addresses of seq and off of the last gather */
	public static native void genomesRegions(long genomes, long[] out);

	public static native void genomesDestroy(long genomes);

	/** gs_accmap_create: knownTaxids = nNodes x int32 ascending; categories / statuses: substrings searched for in fields 4 and 5 */
	public static native long accmapCreate(int device, boolean dna, boolean rna, boolean mrna, String[] categories, String[] statuses,
			ByteBuffer knownTaxids, long knownTaxidsCap, int nNodes, long reserveEntries);

	/** gs_accmap_submit with GS_MEM_HOST; report[8] as the C call's ([3] = 1: refused, the chunk is the caller's) */
	public static native void accmapSubmit(long accmap, ByteBuffer text, long textCap, long nBytes, boolean last, long[] report);

	/** gs_accmap_append: keys32 = n x 32 bytes, nodes = n x int32 */
	public static native void accmapAppend(long accmap, ByteBuffer keys32, long keys32Cap, ByteBuffer nodes, long nodesCap, long n, long nPassing);

	/** gs_accmap_finish: info[4] = entries, passing entries in all, entries equal to the one in front, those with another node */
	public static native void accmapFinish(long accmap, long[] info);

	/** gs_accmap_fetch: keys32 = entries x 32 bytes, nodes = entries x int32, regions = nNodes x int32; any may be null */
	public static native void accmapFetch(long accmap, ByteBuffer keys32, long keys32Cap, ByteBuffer nodes, long nodesCap, ByteBuffer regions,
			long regionsCap);

	/** gs_accmap_lookup with GS_MEM_HOST: headerOff = n + 1 x int64 into headers, nodeOut = n x int32 */
	public static native void accmapLookup(long accmap, ByteBuffer headers, long headersCap, ByteBuffer headerOff, long headerOffCap, long n,
			boolean completeOnly, ByteBuffer nodeOut, long nodeOutCap);

	/** gs_accmap_lookup_genomes: the header lines of the chunk `genomes` has scanned; nodeOut = n_records x int32 */
	public static native void accmapLookupGenomes(long accmap, long genomes, boolean completeOnly, ByteBuffer nodeOut, long nodeOutCap);

	public static native int accmapGetDevice(long accmap);

	/** gs_accmap_get_n_nodes */
	public static native int accmapGetNNodes(long accmap);

	public static native void accmapDestroy(long accmap);

	/** gs_host_accmap_files: the accmapsize (countOnly: returns 0, totals[1] is the number) and accmap goals over catalog files;
	 *  totals[5] = lines, passing, put, device_chunks, host_chunks; returns the finished map */
	public static native long hostAccmapFiles(String[] paths, int device, boolean dna, boolean rna, boolean mrna, String[] categories,
			String[] statuses, ByteBuffer knownTaxids, long knownTaxidsCap, int nNodes, long reserveEntries, boolean countOnly, long[] totals);

	/** gs_asmsum_create: filter = nNodes bytes or null (every node); qualityMask: bit q allows ordinal q, -1 all */
	public static native long asmsumCreate(int device, ByteBuffer knownTaxids, long knownTaxidsCap, int nNodes, ByteBuffer filter, long filterCap,
			int qualityMask, boolean referenceOnly, boolean useSpeciesTaxid, long reserveEntries);

	/** gs_asmsum_submit with GS_MEM_HOST; report[8] as the C call's */
	public static native void asmsumSubmit(long asmsum, ByteBuffer text, long textCap, long nBytes, boolean last, long[] report);

	/** gs_asmsum_append: nodes n x int32, quality / isRef n bytes, lines n x int64, strOff 3 n + 1 x int64 into pool */
	public static native void asmsumAppend(long asmsum, ByteBuffer nodes, long nodesCap, ByteBuffer quality, long qualityCap, ByteBuffer isRef,
			long isRefCap, ByteBuffer lines, long linesCap, ByteBuffer strOff, long strOffCap, ByteBuffer pool, long poolCap, long n, long nCounted,
			long nLines);

	/** gs_asmsum_finish: info[4] = kept entries, picked entries, nodes with entries, counted records */
	public static native void asmsumFinish(long asmsum, int maxPerNode, long[] info);

	/** gs_asmsum_fetch: arrays of `picked` elements as for asmsumAppend; any may be null; pool = strOff[3 x picked] bytes */
	public static native void asmsumFetch(long asmsum, ByteBuffer nodes, long nodesCap, ByteBuffer quality, long qualityCap, ByteBuffer isRef,
			long isRefCap, ByteBuffer lines, long linesCap, ByteBuffer strOff, long strOffCap, ByteBuffer pool, long poolCap);

	/** gs_asmsum_file_name: returns the length of AssemblyEntry's file name of ftp[0, n); min(length, outCap) bytes are written */
	public static native long asmsumFileName(ByteBuffer ftp, long ftpCap, long n, ByteBuffer out, long outCap);

	public static native int asmsumGetDevice(long asmsum);

	public static native void asmsumDestroy(long asmsum);

	/** gs_host_asmsum_files: the fastasgenbank goal over assembly summary files; totals[7] = lines, counted, kept, picked, nodes,
	 *  device_chunks, host_chunks; returns the finished handle (asmsumFetch) */
	public static native long hostAsmsumFiles(String[] paths, int device, ByteBuffer knownTaxids, long knownTaxidsCap, int nNodes, ByteBuffer filter,
			long filterCap, int qualityMask, boolean referenceOnly, boolean useSpeciesTaxid, long reserveEntries, int maxPerNode, long[] totals);

	/** gs_taxtree_create */
	public static native long taxtreeCreate(int device);

	/** gs_taxtree_submit_nodes with GS_MEM_HOST; report[8] as the C call's */
	public static native void taxtreeSubmitNodes(long taxtree, ByteBuffer text, long textCap, long nBytes, boolean last, long[] report);

	public static native void taxtreeAppendNodes(long taxtree, ByteBuffer text, long textCap, long nBytes, boolean last, long[] report);

	/** gs_taxtree_finish_nodes: info[8], [0] = nodes, [1] = nodes the root reaches */
	public static native void taxtreeFinishNodes(long taxtree, long[] info);

	public static native void taxtreeSubmitNames(long taxtree, ByteBuffer text, long textCap, long nBytes, boolean last, long[] report);

	public static native void taxtreeAppendNames(long taxtree, ByteBuffer text, long textCap, long nBytes, boolean last);

	/** gs_taxtree_fetch: nodes x int32 each, any may be null */
	public static native void taxtreeFetch(long taxtree, ByteBuffer taxids, long taxidsCap, ByteBuffer parent, long parentCap, ByteBuffer depth,
			long depthCap, ByteBuffer position, long positionCap, ByteBuffer subtree, long subtreeCap, ByteBuffer rank, long rankCap);

	/** gs_taxtree_fetch_names: offsets = nodes + 1 x int64 (offsets[nodes] = the bytes in all); bytes null: the offsets alone */
	public static native void taxtreeFetchNames(long taxtree, ByteBuffer offsets, long offsetsCap, ByteBuffer bytes, long bytesCap);

	/** gs_taxtree_select: the taxnodes set; out = nodes bytes; returns how many are set */
	public static native long taxtreeSelect(long taxtree, int[] requested, long nRequested, int[] excluded, long nExcluded, int cutRank,
			ByteBuffer out, long outCap);

	/** gs_taxtree_small with GS_MEM_HOST: flagged = nodes x flagBytes (1 or 4); outputs = room for the nodes the root reaches, any may be
	 *  null; returns n_small */
	public static native int taxtreeSmall(long taxtree, ByteBuffer flagged, long flaggedCap, int flagBytes, ByteBuffer nodeOfVi, long nodeOfViCap,
			ByteBuffer parentVi, long parentViCap, ByteBuffer depth, long depthCap, ByteBuffer position, long positionCap);

	/** gs_taxtree_regions_below with GS_MEM_HOST: regions / inclusive = nodes x int32, below = nSelected x int32; returns n_below */
	public static native long taxtreeRegionsBelow(long taxtree, ByteBuffer regions, long regionsCap, int[] selected, long nSelected, int limit,
			int checkRank, ByteBuffer inclusive, long inclusiveCap, ByteBuffer below, long belowCap);

	/** gs_taxtree_read_taxids: counts[2] = requested, excluded ids there are; at most cap of each are written */
	public static native void taxtreeReadTaxids(ByteBuffer text, long textCap, long nBytes, ByteBuffer requested, long requestedCap,
			ByteBuffer excluded, long excludedCap, long cap, long[] counts);

	public static native int taxtreeGetDevice(long taxtree);

	public static native void taxtreeDestroy(long taxtree);

	/** gs_host_taxtree_files: the taxtree goal over nodes.dmp and (unless null) names.dmp; report[8] as the C call's; returns the
	 *  finished tree */
	public static native long hostTaxtreeFiles(int device, String nodesPath, String namesPath, long[] report);

	/** gs_host_read_taxids_file: counts as taxtreeReadTaxids */
	public static native void hostReadTaxidsFile(String path, ByteBuffer requested, long requestedCap, ByteBuffer excluded, long excludedCap,
			long cap, long[] counts);

	/** gs_host_genome_files_into: genome FASTA files straight into a sizer, builder, updater or quality handle.  accmap: a finished
	 *  map or 0 when nodeOfFile gives every file's node; nodeOfFile: null, or per path a node (>= 0: no lookup) or -1; viOfNode =
	 *  nNodes x int32 (< 0: skip); kind: INTO_*; totals[7] = records, kept_records, text_bytes, kept_bases, chunks, host_chunks,
	 *  max_line_bytes.  Limits per tax id and finer nodes are not served. */
	public static native void hostGenomeFilesInto(String[] paths, int device, long accmap, boolean completeOnly, int[] nodeOfFile,
			ByteBuffer viOfNode, long viOfNodeCap, int nNodes, int kind, long handle, boolean update, long[] totals);

	public static final int INTO_SIZE = 0, INTO_BUILD = 1, INTO_UPDATE = 2, INTO_QUALITY = 3;

	// column indices of the integer table (include/gsgpu.h, GS_C_*)
	public static final int C_READS = 0, C_READS_KMERS = 1, C_KMERS = 2, C_UNIQUE_KMERS = 3, C_CONTIGS = 4,
			C_CONTIG_LEN_SQ_SUM = 5, C_MAX_CONTIG_LEN = 6, C_READS_1KMER = 7, C_READS_BPS = 8,
			C_MAX_CONTIG_READ_NO = 9, N_COLS = 10;
	public static final int D_ERR_SUM = 0, D_ERR_SQ_SUM = 1, D_CLASS_ERR_SUM = 2, D_CLASS_ERR_SQ_SUM = 3, N_DCOLS = 4;
	public static final int F_FOUND = 1, F_RETURNED = 2, F_COUNTED = 4;
	public static final int BLOOM_XOR = 0, BLOOM_MURMUR = 1, BLOOM_BLOCKED = 2;
}
