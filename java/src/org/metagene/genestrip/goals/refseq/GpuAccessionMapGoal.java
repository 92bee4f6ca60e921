/*
 * The accmap goal below the JVM: AccessionMapGoal.doMakeThis (reference: core/src/main/java/org/metagene/genestrip/goals/refseq/
 * AccessionMapGoal.java:82-114) walks the RefSeq catalog on one thread, puts every passing entry whose tax id names a node and
 * sorts.  The override loads the tree's tax ids on the device (GpuTaxTree over the nodes.dmp the taxtree goal read), hands the
 * catalog file to gs_host_accmap_files (GsGpuNative.hostAccmapFiles) and fills an AccessionMapImpl from ONE fetch of the sorted
 * slots: put() per entry in the device's order, incRefSeqRegions() per entry as handleEntry does, optimize() over sorted keys.
 * Everything behind the goal -- AbstractRefSeqFastaReader.updateNodeFromInfoLine, TaxNodesFromGenbankGoal -- sees the map and the
 * region counts it would have seen.  One deliberate difference (INTEGRATION.md): among equal accessions the reference's get finds
 * whichever its quicksort left in the way; the slots come with the catalog's first in front.
 * The device map and the per-node counts stay available (deviceMap(), regions()) for GpuTaxNodesFromGenbankGoal and for
 * GpuStoreFastaReader.filesInto until the goal is cleaned.
 * SOURCE ONLY (no JDK in the build container); tools/check_java_glue.py checks the reference members used here.
 */
package org.metagene.genestrip.goals.refseq;

import java.nio.ByteBuffer;
import java.util.List;
import java.util.Set;
import java.util.function.IntSupplier;

import org.metagene.genestrip.GSConfigKey;
import org.metagene.genestrip.GSConfigKey.SeqType;
import org.metagene.genestrip.GSProject;
import org.metagene.genestrip.gpu.GpuAccessionMap;
import org.metagene.genestrip.gpu.GpuTaxTree;
import org.metagene.genestrip.make.Goal;
import org.metagene.genestrip.make.ObjectGoal;
import org.metagene.genestrip.refseq.AccessionMap;
import org.metagene.genestrip.refseq.AccessionMapImpl;
import org.metagene.genestrip.refseq.RefSeqCategory;
import org.metagene.genestrip.tax.TaxTree;
import org.metagene.genestrip.tax.TaxTree.TaxIdNode;

public class GpuAccessionMapGoal<P extends GSProject> extends AccessionMapGoal<P> {
	private final ObjectGoal<Set<RefSeqCategory>, P> categories;
	private final ObjectGoal<TaxTree, P> taxTree;
	private final RefSeqCatalogDownloadGoal catalog;
	private final ObjectGoal<Integer, P> mapSize;
	private final IntSupplier device;
	private GpuTaxTree deviceTree;
	private GpuAccessionMap deviceMap;
	private ByteBuffer regions;

	@SafeVarargs
	public GpuAccessionMapGoal(P project, ObjectGoal<Set<RefSeqCategory>, P> categoriesGoal, ObjectGoal<TaxTree, P> taxTreeGoal,
			RefSeqCatalogDownloadGoal catalogGoal, ObjectGoal<Integer, P> accessionMapSizeGoal, IntSupplier device, Goal<P>... deps) {
		super(project, categoriesGoal, taxTreeGoal, catalogGoal, accessionMapSizeGoal, deps);
		this.categories = categoriesGoal;
		this.taxTree = taxTreeGoal;
		this.catalog = catalogGoal;
		this.mapSize = accessionMapSizeGoal;
		this.device = device;
	}

	/** the tree on the device, node = index of the tax id; null before the goal is made */
	public GpuTaxTree deviceTree() {
		return deviceTree;
	}

	/** the map on the device: what GsGpuNative.hostGenomeFilesInto looks header lines up in; null before the goal is made */
	public GpuAccessionMap deviceMap() {
		return deviceMap;
	}

	/** entries per node itself, nodes x int32: what gs_taxtree_regions_below takes; null before the goal is made */
	public ByteBuffer regions() {
		return regions;
	}

	@Override
	@SuppressWarnings("unchecked")
	protected void doMakeThis() {
		SeqType seqType = (SeqType) configValue(GSConfigKey.SEQ_TYPE);
		List<GSConfigKey.RefSeqStatus> statuses = (List<GSConfigKey.RefSeqStatus>) configValue(GSConfigKey.RES_SEQ_STATUS);
		TaxTree tree = taxTree.get();
		release();
		deviceTree = GpuTaxTree.load(device.getAsInt(), getProject().getCommon().getCommonDir(), false);
		int[] taxIds = deviceTree.taxIds();
		deviceMap = GpuAccessionMap.fromCatalogs(new String[] { catalog.getCatalogFile().getPath() }, device.getAsInt(),
				GpuAccessionMapSizeGoal.dna(seqType), GpuAccessionMapSizeGoal.rna(seqType), GpuAccessionMapSizeGoal.mrna(seqType),
				GpuAccessionMapSizeGoal.categoryStrings(categories.get()), GpuAccessionMapSizeGoal.statusStrings(statuses),
				deviceTree.taxIdBuffer(), taxIds.length, mapSize.get());
		regions = deviceMap.regions();
		if (deviceMap.entries() > Integer.MAX_VALUE / GpuAccessionMap.SLOT) {
			throw new IllegalStateException("more entries than one fetch into a ByteBuffer holds: " + deviceMap.entries());
		}
		int n = (int) deviceMap.entries();
		ByteBuffer keys = deviceMap.keys();
		ByteBuffer nodes = deviceMap.nodes();
		AccessionMap map = new AccessionMapImpl(n);
		TaxIdNode[] nodeOf = new TaxIdNode[taxIds.length];
		byte[] slot = new byte[GpuAccessionMap.SLOT];
		for (int i = 0; i < n; i++) {
			keys.position(GpuAccessionMap.SLOT * i);
			keys.get(slot);
			int index = nodes.getInt(4 * i);
			TaxIdNode node = nodeOf[index];
			if (node == null) {
				node = tree.getNodeByTaxId(Integer.toString(taxIds[index]));
				nodeOf[index] = node;
			}
			if (node != null) {
				map.put(slot, 1, 1 + slot[0], node);
				node.incRefSeqRegions();
			}
		}
		map.optimize();
		set(map);
	}

	private void release() {
		if (deviceMap != null) {
			deviceMap.close();
			deviceMap = null;
		}
		if (deviceTree != null) {
			deviceTree.close();
			deviceTree = null;
		}
		regions = null;
	}

	@Override
	protected void doCleanThis() {
		release();
		super.doCleanThis();
	}
}
