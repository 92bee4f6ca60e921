/*
 * The accmapsize goal below the JVM: AccessionMapSizeGoal.doMakeThis (reference: core/src/main/java/org/metagene/genestrip/goals/
 * refseq/AccessionMapSizeGoal.java:70-103) walks the RefSeq catalog on one thread and counts the entries that pass; the override
 * hands the catalog file to gs_host_accmap_files with count_only (GsGpuNative.hostAccmapFiles): chunks of whole lines scanned on the
 * device, what it refuses line by line in the host layer, the same number.  The categories and statuses travel as the strings
 * AccessionFileProcessor searches for (RefSeqCategory.getDirectory, RefSeqStatus.getName), SeqType as its three flags
 * (refseq/AccessionFileProcessor.java:79-88).
 * SOURCE ONLY (no JDK in the build container); tools/check_java_glue.py checks the reference members used here.
 */
package org.metagene.genestrip.goals.refseq;

import java.util.List;
import java.util.Set;
import java.util.function.IntSupplier;

import org.metagene.genestrip.GSConfigKey;
import org.metagene.genestrip.GSConfigKey.SeqType;
import org.metagene.genestrip.GSProject;
import org.metagene.genestrip.gpu.GpuAccessionMap;
import org.metagene.genestrip.make.Goal;
import org.metagene.genestrip.make.ObjectGoal;
import org.metagene.genestrip.refseq.RefSeqCategory;

public class GpuAccessionMapSizeGoal<P extends GSProject> extends AccessionMapSizeGoal<P> {
	private final ObjectGoal<Set<RefSeqCategory>, P> categories;
	private final RefSeqCatalogDownloadGoal catalog;
	// a supplier, not an int: GSMaker creates its goals inside the superclass constructor, before a subclass's fields are set
	private final IntSupplier device;

	@SafeVarargs
	public GpuAccessionMapSizeGoal(P project, ObjectGoal<Set<RefSeqCategory>, P> categoriesGoal, RefSeqCatalogDownloadGoal catalogGoal,
			IntSupplier device, Goal<P>... deps) {
		super(project, categoriesGoal, catalogGoal, deps);
		this.categories = categoriesGoal;
		this.catalog = catalogGoal;
		this.device = device;
	}

	static String[] categoryStrings(Set<RefSeqCategory> categories) {
		String[] res = new String[categories.size()];
		int i = 0;
		for (RefSeqCategory category : categories) {
			res[i++] = category.getDirectory();
		}
		return res;
	}

	static String[] statusStrings(List<GSConfigKey.RefSeqStatus> statuses) {
		String[] res = new String[statuses.size()];
		for (int i = 0; i < res.length; i++) {
			res[i] = statuses.get(i).getName();
		}
		return res;
	}

	static boolean dna(SeqType t) {
		return SeqType.GENOMIC.equals(t) || SeqType.ALL.equals(t);
	}

	static boolean rna(SeqType t) {
		return SeqType.RNA.equals(t) || SeqType.ALL.equals(t) || SeqType.ALL_RNA.equals(t);
	}

	static boolean mrna(SeqType t) {
		return SeqType.M_RNA.equals(t) || SeqType.ALL.equals(t) || SeqType.ALL_RNA.equals(t);
	}

	@Override
	@SuppressWarnings("unchecked")
	protected void doMakeThis() {
		SeqType seqType = (SeqType) configValue(GSConfigKey.SEQ_TYPE);
		List<GSConfigKey.RefSeqStatus> statuses = (List<GSConfigKey.RefSeqStatus>) configValue(GSConfigKey.RES_SEQ_STATUS);
		long n = GpuAccessionMap.countPassing(new String[] { catalog.getCatalogFile().getPath() }, device.getAsInt(), dna(seqType), rna(seqType),
				mrna(seqType), categoryStrings(categories.get()), statusStrings(statuses));
		if (n > Integer.MAX_VALUE) {
			throw new IllegalStateException("more catalog entries than an AccessionMapImpl holds: " + n);
		}
		set((int) n);
		if (getLogger().isDebugEnabled()) {
			getLogger().debug("Map size determined: " + n);
		}
	}
}
