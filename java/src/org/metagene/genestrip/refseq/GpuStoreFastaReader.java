/*
 * Reference-side glue for gs_dbbuild (include/gsgpu.h): the FASTA reader of FillDBGoal / DBGoal with the k-mer work moved to
 * the GPU.  Source only -- there is no JDK in the build image; tools/check_java_glue.py checks every member this class
 * touches against the reference's sources.
 *
 * The reference's readers (FillDBGoal.MyFastaReader, DBGoal.MyFastaReader; both AbstractStoreFastaReader) push every base
 * through a CGATLongBuffer and call store.put / store.update per k-mer (refseq/AbstractStoreFastaReader.java:87-115).  This
 * reader keeps everything that decides WHICH regions count and under WHICH node -- infoLine(), the accession map, the
 * per-taxid limits, reworkNode(): all inherited -- and only collects the bases of the included regions; a full buffer goes
 * to the device as one batch of regions (GsGpuNative.dbBuildAdd).  After the last file of the fill pass and of the update pass
 * the goal calls finish(), which returns the sorted k-mers and value indices a KMerSortedArray / gs_db_create takes.
 */
package org.metagene.genestrip.refseq;

import java.io.File;
import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.util.List;
import java.util.Map;
import java.util.Set;

import org.metagene.genestrip.gpu.GpuAccessionMap;
import org.metagene.genestrip.gpu.GpuTaxTree;
import org.metagene.genestrip.gpu.GsGpuNative;
import org.metagene.genestrip.tax.Rank;
import org.metagene.genestrip.tax.TaxTree;
import org.metagene.genestrip.tax.TaxTree.TaxIdNode;

public class GpuStoreFastaReader extends AbstractRefSeqFastaReader {
	private final long builder;
	private long updater;
	private long sizer;
	private final boolean update;
	private final boolean allRegions;
	private final Map<TaxIdNode, Integer> valueIndexOfNode;
	private final ByteBuffer bases;
	private final ByteBuffer offsets;
	private final ByteBuffer nodes;
	private final int maxRegions;
	private final boolean completeOnly;
	private int regions;
	private boolean open;

	/**
	 * @param builder          handle of GsGpuNative.dbBuildBegin (shared by the fill and the update reader)
	 * @param update           false: FillDBGoal (regions of the requested taxa are stored), true: DBGoal (LCA updates)
	 * @param allRegions       DBGoal without minUpdate: every region with a node counts (goals/refseq/DBGoal.java:267-283)
	 * @param valueIndexOfNode the value index every tree node got when the tree was handed to dbBuildBegin
	 * @param batchBytes       bases collected before a batch goes to the device
	 */
	public GpuStoreFastaReader(long builder, boolean update, boolean allRegions, Map<TaxIdNode, Integer> valueIndexOfNode,
			int batchBytes, int bufferSize, Set<TaxIdNode> taxNodes, AccessionMap accessionMap, int k, int maxGenomesPerTaxId,
			Rank maxGenomesPerTaxIdRank, long maxKmersPerTaxId, int stepSize, boolean completeGenomesOnly,
			StringLong2DigitTrie regionsPerTaxid) {
		super(bufferSize, taxNodes, accessionMap, k, maxGenomesPerTaxId, maxGenomesPerTaxIdRank, maxKmersPerTaxId, stepSize,
				completeGenomesOnly, regionsPerTaxid);
		this.builder = builder;
		this.update = update;
		this.allRegions = allRegions;
		this.valueIndexOfNode = valueIndexOfNode;
		this.maxRegions = Math.max(1024, batchBytes / 256);
		this.completeOnly = completeGenomesOnly;
		this.bases = ByteBuffer.allocateDirect(batchBytes);
		this.offsets = ByteBuffer.allocateDirect(8 * (maxRegions + 1)).order(ByteOrder.nativeOrder());
		this.nodes = ByteBuffer.allocateDirect(4 * maxRegions).order(ByteOrder.nativeOrder());
		this.offsets.putLong(0, 0L);
	}

	/**
	 * The update pass as a stream past a finished store: the regions go to an updater handle (GsGpuNative.dbUpdateBegin /
	 * dbUpdateBeginDb) in place of a builder handle, batch by batch; nothing stays on the device but the store.  Only for the
	 * update pass: the reader is one with update = true.
	 */
	public static GpuStoreFastaReader forUpdater(long updater, boolean allRegions, Map<TaxIdNode, Integer> valueIndexOfNode,
			int batchBytes, int bufferSize, Set<TaxIdNode> taxNodes, AccessionMap accessionMap, int k, int maxGenomesPerTaxId,
			Rank maxGenomesPerTaxIdRank, long maxKmersPerTaxId, int stepSize, boolean completeGenomesOnly,
			StringLong2DigitTrie regionsPerTaxid) {
		GpuStoreFastaReader reader = new GpuStoreFastaReader(0L, true, allRegions, valueIndexOfNode, batchBytes, bufferSize, taxNodes,
				accessionMap, k, maxGenomesPerTaxId, maxGenomesPerTaxIdRank, maxKmersPerTaxId, stepSize, completeGenomesOnly,
				regionsPerTaxid);
		reader.updater = updater;
		return reader;
	}

	/**
	 * The sizing walks in front of the fill pass (FillSizeGoal, FillBloomFilterGoal): the regions of the requested taxa go to a
	 * sizer handle (GsGpuNative.dbSizeBegin) in place of a builder handle, tagged with their node's value index; the goal reads
	 * GsGpuNative.dbSizeCounts / dbSizeDistinct after the last file.  The reader is one with update = false.
	 */
	public static GpuStoreFastaReader forSizer(long sizer, Map<TaxIdNode, Integer> valueIndexOfNode, int batchBytes, int bufferSize,
			Set<TaxIdNode> taxNodes, AccessionMap accessionMap, int k, int maxGenomesPerTaxId, Rank maxGenomesPerTaxIdRank,
			long maxKmersPerTaxId, int stepSize, boolean completeGenomesOnly, StringLong2DigitTrie regionsPerTaxid) {
		GpuStoreFastaReader reader = new GpuStoreFastaReader(0L, false, false, valueIndexOfNode, batchBytes, bufferSize, taxNodes,
				accessionMap, k, maxGenomesPerTaxId, maxGenomesPerTaxIdRank, maxKmersPerTaxId, stepSize, completeGenomesOnly,
				regionsPerTaxid);
		reader.sizer = sizer;
		return reader;
	}

	@Override
	protected void infoLine() {
		super.infoLine();
		if (update && allRegions) {
			// DBGoal.MyFastaReader.infoLine: without minUpdate every region is walked, under its own node if it has one
			includeRegion = true;
			if (node != null) {
				node = reworkNode();
			}
		}
		open = includeRegion && node != null && valueIndexOfNode.containsKey(node);
		if (open && regions == maxRegions) {
			flush();
		}
	}

	@Override
	protected void dataLine() {
		if (!open || !isAllowMoreKmers()) {
			return;
		}
		// the line without its terminator(s), as AbstractStoreFastaReader.dataLine strips them
		int end = size;
		while (end > 0 && (target[end - 1] == '\n' || target[end - 1] == '\r')) {
			end--;
		}
		if (end > bases.remaining()) {
			// the region goes on in the next batch: a region border resets the k-mer window, so the last k - 1 bases are
			// handed in again in front of the rest (they form no k-mer by themselves).  (With stepSize > 1 the positions
			// that are sampled are counted from the region start: give such builds a batch that holds the longest region.)
			int keep = Math.min(k - 1, bases.position() - (int) offsets.getLong(8 * regions));
			byte[] tail = new byte[keep];
			for (int i = 0; i < keep; i++) {
				tail[i] = bases.get(bases.position() - keep + i);
			}
			closeRegion();
			flush();
			bases.put(tail);
		}
		bases.put(target, 0, end);
		bpsInRegion += end;
	}

	@Override
	protected void endRegion() {
		if (open) {
			closeRegion();
			open = false;
		}
		super.endRegion();
	}

	private void closeRegion() {
		nodes.putInt(4 * regions, valueIndexOfNode.get(node));
		regions++;
		offsets.putLong(8 * regions, bases.position());
	}

	/**
	 * The files of a pass without this reader's line walk: gs_host_genome_files_into (GsGpuNative.hostGenomeFilesInto) cuts them into
	 * chunks of whole records, finds the records and gathers the bases on the device, looks the header lines up in the device map
	 * where the scan left them and hands the kept regions to this reader's handle -- sizer, updater or builder -- in device memory.
	 * What infoLine() decides travels as a table: per node of the device tree the value index, or -1 where infoLine() would not
	 * include the region (taxNodes, valueIndexOfNode; with update and allRegions every node that has a value index).
	 *
	 * The call does not serve what needs a look at every record in file order: a limit (maxGenomesPerTaxId / maxKMersPerTaxId below
	 * their maxima -- maxGenomesPerTaxIdRank only matters with one) or finer nodes (idNodes / fileNodes / dataNodes: the caller says so,
	 * reworkNode() is the goal's).  Then, and for a file node the dump does not hold, nothing is done and false comes back: the
	 * caller reads the files with readFasta() as before.  regionsPerTaxid is not counted on this path (nothing reads it without a
	 * limit), and the reference's "buffer is too small for data line" is not raised: totals[6] holds the longest line.
	 *
	 * @param files      the pass's FASTA files in order (plain, gzip or BGZF)
	 * @param fileNodes  null, or per file the node of ignoreAccessionMap(node) for an additional FASTA file and null for a RefSeq file
	 * @param tree       the tree the value indices were made from
	 * @param deviceTree the same dump on the device: its node indices are the map's
	 * @param deviceMap  the accession map on the device, or null if every file has a node
	 * @param finerNodes true if idNodes, fileNodes or dataNodes is configured
	 * @param totals     null, or long[7] as GsGpuNative.hostGenomeFilesInto fills it
	 * @return true if the files went through the call
	 */
	public boolean filesInto(int device, List<File> files, List<TaxIdNode> fileNodes, TaxTree tree, GpuTaxTree deviceTree, GpuAccessionMap deviceMap,
			boolean finerNodes, long[] totals) {
		if (finerNodes || maxGenomesPerTaxId != Integer.MAX_VALUE || maxKmersPerTaxId != Long.MAX_VALUE) {
			return false;
		}
		String[] paths = new String[files.size()];
		int[] nodeOfFile = new int[paths.length];
		for (int i = 0; i < paths.length; i++) {
			paths[i] = files.get(i).getPath();
			TaxIdNode given = fileNodes == null ? null : fileNodes.get(i);
			nodeOfFile[i] = given == null ? -1 : deviceTree.nodeOf(given.getTaxId());
			if ((given != null && nodeOfFile[i] < 0) || (given == null && deviceMap == null)) {
				return false;
			}
		}
		int[] taxIds = deviceTree.taxIds();
		ByteBuffer viOfNode = ByteBuffer.allocateDirect(4 * Math.max(taxIds.length, 1)).order(ByteOrder.nativeOrder());
		for (int i = 0; i < taxIds.length; i++) {
			TaxIdNode n = tree.getNodeByTaxId(Integer.toString(taxIds[i]));
			Integer vi = n == null ? null : valueIndexOfNode.get(n);
			boolean wanted = (update && allRegions) || taxNodes.isEmpty() || taxNodes.contains(n);
			viOfNode.putInt(4 * i, vi != null && wanted ? vi : -1);
		}
		flush();
		int kind = sizer != 0L ? GsGpuNative.INTO_SIZE : updater != 0L ? GsGpuNative.INTO_UPDATE : GsGpuNative.INTO_BUILD;
		long handle = sizer != 0L ? sizer : updater != 0L ? updater : builder;
		GsGpuNative.hostGenomeFilesInto(paths, device, deviceMap == null ? 0L : deviceMap.handle(), completeOnly, nodeOfFile, viOfNode, taxIds.length,
				taxIds.length, kind, handle, update, totals == null ? new long[7] : totals);
		return true;
	}

	/** hands the collected regions to the device (also called by the goal after the last file of a pass) */
	public void flush() {
		if (regions > 0) {
			if (sizer != 0L) {
				GsGpuNative.dbSizeAdd(sizer, bases, offsets, nodes, regions);
			} else if (updater != 0L) {
				GsGpuNative.dbUpdateAdd(updater, bases, offsets, nodes, regions);
			} else {
				GsGpuNative.dbBuildAdd(builder, bases, offsets, nodes, regions, update);
			}
		}
		bases.clear();
		regions = 0;
		offsets.putLong(0, 0L);
	}
}
