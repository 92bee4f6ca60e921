/*
 * The one place where the GPU goals enter the goal graph: GSMaker builds the chains for `match` and `filter` in two
 * protected factory methods (reference: core/src/main/java/org/metagene/genestrip/GSMaker.java:560-583 and :601-625);
 * the overrides repeat them with GpuMatchResultGoal / GpuFilterGoal as the last link.  Use it wherever the reference
 * creates a GSMaker (Main, API users): `new GpuGSMaker<>(project, device)`.  SOURCE ONLY (no JDK in the build container).
 *
 * `extract` and `fasta2fastq` have no factory method: GSMaker.createGoals constructs them inline (:433-434, :472-473) and
 * hands them to registerGoal.  The override of registerGoal puts GpuExtractGoal / GpuFasta2FastqGoal in their place, built
 * from the same goals, which createGoals has registered by then (FASTQ_MAP_TRANSFORM; FASTA_MAP_TRANSFORM, SETUP,
 * FASTA_DOWNLOAD).  createGoals runs inside Maker's constructor, before `device` is assigned here, so the two goals take the
 * device as a supplier and read it when they are made.
 *
 * The database chain enters the same way: `accmapsize`, `accmap`, `taxfromgenbank` and `fastasgenbank` are constructed inline too
 * (:269-287), each from the goal in front of it.  registerGoal puts GpuAccessionMapSizeGoal, GpuAccessionMapGoal,
 * GpuTaxNodesFromGenbankGoal and GpuFastaFilesFromGenbankGoal in their place, each built from the goals REGISTERED by then, so the
 * four hang together and a goal made by its key runs on the device.  What createGoals builds behind them (fastasgenbankdl, fillsize,
 * filldb, db, ...) got the reference's instances as constructor arguments before registerGoal saw them and keeps those: the seam for
 * them is a factory method upstream, as match and filter have one.
 */
package org.metagene.genestrip;

import java.util.Map;
import java.util.Set;

import org.metagene.genestrip.goals.ExtractGoal;
import org.metagene.genestrip.goals.Fasta2FastqGoal;
import org.metagene.genestrip.goals.FastqDownloadsGoal;
import org.metagene.genestrip.goals.FastqMapGoal;
import org.metagene.genestrip.goals.FastqMapTransformGoal;
import org.metagene.genestrip.goals.FilterGoal;
import org.metagene.genestrip.goals.GpuExtractGoal;
import org.metagene.genestrip.goals.GpuFasta2FastqGoal;
import org.metagene.genestrip.goals.GpuFilterGoal;
import org.metagene.genestrip.goals.GpuMatchResultGoal;
import org.metagene.genestrip.goals.LoadDBGoal;
import org.metagene.genestrip.goals.LoadIndexGoal;
import org.metagene.genestrip.goals.MatchResultGoal;
import org.metagene.genestrip.goals.genbank.FastaFilesFromGenbankGoal;
import org.metagene.genestrip.goals.genbank.GpuFastaFilesFromGenbankGoal;
import org.metagene.genestrip.goals.genbank.GpuTaxNodesFromGenbankGoal;
import org.metagene.genestrip.goals.genbank.TaxNodesFromGenbankGoal;
import org.metagene.genestrip.goals.refseq.AccessionMapGoal;
import org.metagene.genestrip.goals.refseq.AccessionMapSizeGoal;
import org.metagene.genestrip.goals.refseq.GpuAccessionMapGoal;
import org.metagene.genestrip.goals.refseq.GpuAccessionMapSizeGoal;
import org.metagene.genestrip.goals.refseq.RefSeqCatalogDownloadGoal;
import org.metagene.genestrip.io.StreamingResourceStream;
import org.metagene.genestrip.make.FileGoal;
import org.metagene.genestrip.make.Goal;
import org.metagene.genestrip.make.ObjectGoal;
import org.metagene.genestrip.refseq.AccessionMap;
import org.metagene.genestrip.refseq.RefSeqCategory;
import org.metagene.genestrip.tax.TaxTree;
import org.metagene.genestrip.tax.TaxTree.TaxIdNode;

public class GpuGSMaker<P extends GSProject> extends GSMaker<P> {
	private final int device;

	public GpuGSMaker(P project, int device) {
		super(project);
		this.device = device;
	}

	@Override
	@SuppressWarnings({ "unchecked", "rawtypes" })
	protected void registerGoal(Goal<P> goal) {
		if (goal instanceof ExtractGoal && !(goal instanceof GpuExtractGoal)) {
			goal = new GpuExtractGoal<P>(getProject(),
					(ObjectGoal<Map<String, StreamingResourceStream>, P>) (ObjectGoal) getGoal(GSGoalKey.FASTQ_MAP_TRANSFORM),
					getExecutionContext(getProject()), () -> device);
		} else if (goal instanceof Fasta2FastqGoal && !(goal instanceof GpuFasta2FastqGoal)) {
			goal = new GpuFasta2FastqGoal<P>(getProject(), goal.getKey(),
					(ObjectGoal<Map<String, StreamingResourceStream>, P>) (ObjectGoal) getGoal(GSGoalKey.FASTA_MAP_TRANSFORM),
					() -> device, getGoal(GSGoalKey.SETUP), getGoal(GSGoalKey.FASTA_DOWNLOAD));
		} else if (goal instanceof AccessionMapSizeGoal && !(goal instanceof GpuAccessionMapSizeGoal)) {
			goal = new GpuAccessionMapSizeGoal<P>(getProject(),
					(ObjectGoal<Set<RefSeqCategory>, P>) (ObjectGoal) getGoal(GSGoalKey.CATEGORIES),
					(RefSeqCatalogDownloadGoal) getGoal(GSGoalKey.REFSEQCAT), () -> device);
		} else if (goal instanceof AccessionMapGoal && !(goal instanceof GpuAccessionMapGoal)) {
			goal = new GpuAccessionMapGoal<P>(getProject(),
					(ObjectGoal<Set<RefSeqCategory>, P>) (ObjectGoal) getGoal(GSGoalKey.CATEGORIES),
					(ObjectGoal<TaxTree, P>) (ObjectGoal) getGoal(GSGoalKey.TAXTREE), (RefSeqCatalogDownloadGoal) getGoal(GSGoalKey.REFSEQCAT),
					(ObjectGoal<Integer, P>) (ObjectGoal) getGoal(GSGoalKey.ACCMAPSIZE), () -> device);
		} else if (goal instanceof TaxNodesFromGenbankGoal && !(goal instanceof GpuTaxNodesFromGenbankGoal)) {
			goal = new GpuTaxNodesFromGenbankGoal<P>(getProject(),
					(ObjectGoal<Set<RefSeqCategory>, P>) (ObjectGoal) getGoal(GSGoalKey.CATEGORIES),
					(ObjectGoal<Set<TaxIdNode>, P>) (ObjectGoal) getGoal(GSGoalKey.TAXNODES),
					(ObjectGoal<AccessionMap, P>) (ObjectGoal) getGoal(GSGoalKey.ACCMAP));
		} else if (goal instanceof FastaFilesFromGenbankGoal && !(goal instanceof GpuFastaFilesFromGenbankGoal)) {
			goal = new GpuFastaFilesFromGenbankGoal<P>(getProject(), (ObjectGoal<TaxTree, P>) (ObjectGoal) getGoal(GSGoalKey.TAXTREE),
					(FileGoal<P>) getGoal(GSGoalKey.ASSEMBLYDOWNLOAD),
					(ObjectGoal<Set<TaxIdNode>, P>) (ObjectGoal) getGoal(GSGoalKey.TAXFROMGENBANK), () -> device);
		}
		super.registerGoal(goal);
	}

	@Override
	@SuppressWarnings({ "unchecked", "rawtypes" })
	protected MatchResultGoal<P> createGoalChainForMatchResult(boolean lr, String key, String... pathsOrURLs) {
		ObjectGoal<Map<String, StreamingResourceStream>, P> fastqMapGoal = new FastqMapGoal(getProject(), true,
				getGoal(GSGoalKey.SETUP)) {
			@Override
			protected void doMakeThis() {
				Map<String, StreamingResourceStream> map = createFastqMap(key, pathsOrURLs, null, null, null);
				set(map);
			}
		};
		ObjectGoal<Map<String, StreamingResourceStream>, P> fastqMapTransfGoal = new FastqMapTransformGoal(getProject(),
				true, fastqMapGoal, getGoal(GSGoalKey.SETUP));
		FastqDownloadsGoal<P> fastqDownloadsGoal = new FastqDownloadsGoal(getProject(), true, fastqMapGoal,
				fastqMapTransfGoal, getGoal(GSGoalKey.SETUP));
		LoadDBGoal<P> loadDBGoal = getLoadDBGoal();
		return new GpuMatchResultGoal<P>(getProject(), (lr ? GSGoalKey.MATCHRESLR : GSGoalKey.MATCHRES),
				fastqMapTransfGoal, loadDBGoal, getExecutionContext(getProject()), device, getGoal(GSGoalKey.SETUP),
				fastqDownloadsGoal);
	}

	@Override
	@SuppressWarnings({ "unchecked", "rawtypes" })
	protected FilterGoal<P> createGoalChainForFilter(String key, String... pathsOrURLs) {
		ObjectGoal<Map<String, StreamingResourceStream>, P> fastqMapGoal = new FastqMapGoal(getProject(), true,
				getGoal(GSGoalKey.SETUP)) {
			@Override
			protected void doMakeThis() {
				Map<String, StreamingResourceStream> map = createFastqMap(key, pathsOrURLs, null, null, null);
				set(map);
			}
		};
		ObjectGoal<Map<String, StreamingResourceStream>, P> fastqMapTransfGoal = new FastqMapTransformGoal(getProject(),
				true, fastqMapGoal, getGoal(GSGoalKey.SETUP));
		FastqDownloadsGoal<P> fastqDownloadsGoal = new FastqDownloadsGoal(getProject(), true, fastqMapGoal,
				fastqMapTransfGoal, getGoal(GSGoalKey.SETUP));
		LoadIndexGoal<P> bloomIndexedGoal = (LoadIndexGoal) getGoal(GSGoalKey.LOAD_INDEX);
		return new GpuFilterGoal<P>(getProject(), fastqMapTransfGoal, bloomIndexedGoal, getExecutionContext(getProject()),
				device, getGoal(GSGoalKey.SETUP), fastqDownloadsGoal);
	}
}
