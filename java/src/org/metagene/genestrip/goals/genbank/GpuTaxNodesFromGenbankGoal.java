/*
 * The taxfromgenbank goal on the device: TaxNodesFromGenbankGoal.doMakeThis (reference: core/src/main/java/org/metagene/genestrip/
 * goals/genbank/TaxNodesFromGenbankGoal.java:72-95) asks every node of the taxnodes set for getRefSeqRegions() -- the count that
 * AccessionMapGoal's incRefSeqRegions walked up the parent chain once per catalog entry.  With a GpuAccessionMapGoal in front the
 * per-node counts are still on hand as one array; gs_taxtree_regions_below (GsGpuNative.taxtreeRegionsBelow) sums them over every
 * subtree with one scan and answers the selected nodes of the checked rank whose count is below the limit.  What the goal puts in
 * front of its loop (refseq.filldb off, SeqType.RNA, limit <= 0) stays here, as in the reference.  An accession map goal of
 * another kind: the reference's loop (super.doMakeThis()).
 * SOURCE ONLY (no JDK in the build container); tools/check_java_glue.py checks the reference members used here.
 */
package org.metagene.genestrip.goals.genbank;

import java.util.ArrayList;
import java.util.HashSet;
import java.util.List;
import java.util.Set;

import org.metagene.genestrip.GSConfigKey;
import org.metagene.genestrip.GSConfigKey.SeqType;
import org.metagene.genestrip.GSProject;
import org.metagene.genestrip.goals.refseq.GpuAccessionMapGoal;
import org.metagene.genestrip.gpu.GpuTaxTree;
import org.metagene.genestrip.make.Goal;
import org.metagene.genestrip.make.ObjectGoal;
import org.metagene.genestrip.refseq.AccessionMap;
import org.metagene.genestrip.refseq.RefSeqCategory;
import org.metagene.genestrip.tax.Rank;
import org.metagene.genestrip.tax.TaxTree.TaxIdNode;

public class GpuTaxNodesFromGenbankGoal<P extends GSProject> extends TaxNodesFromGenbankGoal<P> {
	private final ObjectGoal<Set<TaxIdNode>, P> taxNodes;
	private final ObjectGoal<AccessionMap, P> accessionMap;

	@SafeVarargs
	public GpuTaxNodesFromGenbankGoal(P project, ObjectGoal<Set<RefSeqCategory>, P> categoriesGoal, ObjectGoal<Set<TaxIdNode>, P> taxNodesGoal,
			ObjectGoal<AccessionMap, P> accessionMapGoal, Goal<P>... deps) {
		super(project, categoriesGoal, taxNodesGoal, accessionMapGoal, deps);
		this.taxNodes = taxNodesGoal;
		this.accessionMap = accessionMapGoal;
	}

	@Override
	protected void doMakeThis() {
		int limit = intConfigValue(GSConfigKey.REQ_SEQ_LIMIT_FOR_GENBANK);
		if (!(accessionMap instanceof GpuAccessionMapGoal) || !booleanConfigValue(GSConfigKey.REF_SEQ_DB)
				|| SeqType.RNA.equals(configValue(GSConfigKey.SEQ_TYPE)) || limit <= 0) {
			super.doMakeThis();
			return;
		}
		accessionMap.get();
		GpuAccessionMapGoal<P> made = (GpuAccessionMapGoal<P>) accessionMap;
		GpuTaxTree tree = made.deviceTree();
		Rank checkRank = (Rank) configValue(GSConfigKey.REQ_SEQ_LIMIT_FOR_GENBANK_RANK);
		List<TaxIdNode> asked = new ArrayList<TaxIdNode>();
		List<Integer> index = new ArrayList<Integer>();
		for (TaxIdNode node : taxNodes.get()) {
			int i = tree.nodeOf(node.getTaxId());
			if (i >= 0) {
				asked.add(node);
				index.add(i);
			} else if ((checkRank == null || checkRank.equals(node.getRank())) && node.getRefSeqRegions() < limit) {
				asked.add(node); // (a node the dump does not hold: the reference's own test)
				index.add(-1);
			}
		}
		int[] selected = new int[index.size()];
		int m = 0;
		for (int i : index) {
			if (i >= 0) {
				selected[m++] = i;
			}
		}
		int[] sel = new int[m];
		System.arraycopy(selected, 0, sel, 0, m);
		int[] below = tree.regionsBelow(made.regions(), sel, limit, checkRank == null ? -1 : checkRank.ordinal());
		Set<Integer> hit = new HashSet<Integer>();
		for (int i : below) {
			hit.add(i);
		}
		Set<TaxIdNode> missing = new HashSet<TaxIdNode>();
		for (int i = 0; i < asked.size(); i++) {
			if (index.get(i) < 0 || hit.contains(index.get(i))) {
				missing.add(asked.get(i));
			}
		}
		set(missing);
	}
}
