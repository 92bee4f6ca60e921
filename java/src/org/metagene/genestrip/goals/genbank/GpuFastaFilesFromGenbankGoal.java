/*
 * The fastasgenbank goal below the JVM: FastaFilesFromGenbankGoal.doMakeThis (reference: core/src/main/java/org/metagene/genestrip/
 * goals/genbank/FastaFilesFromGenbankGoal.java:101-150) reads Genbank's assembly summary record by record through
 * AssemblySummaryReader.getRelevantEntries and then cuts every node's list to maxFromGenbank, best quality last.  The override hands
 * the file to gs_host_asmsum_files (GsGpuNative.hostAsmsumFiles): the taxfromgenbank set as one flag per node of the device tree,
 * genbank.fastaQualities as a mask of AssemblyQuality ordinals, the cap applied on the device; one fetch gives the picks per node
 * in the reference's list order, and an AssemblyEntry is made of each as getRelevantEntries makes it.  The goal's early exit on an
 * empty set and the weak dependency on the download stay as they are.
 * SOURCE ONLY (no JDK in the build container); tools/check_java_glue.py checks the reference members used here.
 */
package org.metagene.genestrip.goals.genbank;

import java.io.File;
import java.nio.ByteBuffer;
import java.util.ArrayList;
import java.util.Collections;
import java.util.HashMap;
import java.util.List;
import java.util.Map;
import java.util.Set;
import java.util.function.IntSupplier;

import org.metagene.genestrip.GSConfigKey;
import org.metagene.genestrip.GSProject;
import org.metagene.genestrip.genbank.AssemblySummaryReader;
import org.metagene.genestrip.genbank.AssemblySummaryReader.AssemblyEntry;
import org.metagene.genestrip.genbank.AssemblySummaryReader.AssemblyQuality;
import org.metagene.genestrip.gpu.GpuAssemblySummary;
import org.metagene.genestrip.gpu.GpuTaxTree;
import org.metagene.genestrip.make.FileGoal;
import org.metagene.genestrip.make.ObjectGoal;
import org.metagene.genestrip.tax.TaxTree;
import org.metagene.genestrip.tax.TaxTree.TaxIdNode;

public class GpuFastaFilesFromGenbankGoal<P extends GSProject> extends FastaFilesFromGenbankGoal<P> {
	private final FileGoal<P> assembly;
	private final ObjectGoal<TaxTree, P> taxTree;
	private final ObjectGoal<Set<TaxIdNode>, P> fromGenbank;
	// a supplier, not an int: GSMaker creates its goals inside the superclass constructor, before a subclass's fields are set
	private final IntSupplier device;

	public GpuFastaFilesFromGenbankGoal(P project, ObjectGoal<TaxTree, P> taxTreeGoal, FileGoal<P> assemblyGoal,
			ObjectGoal<Set<TaxIdNode>, P> taxidsFromGenbankGoal, IntSupplier device) {
		super(project, taxTreeGoal, assemblyGoal, taxidsFromGenbankGoal);
		this.assembly = assemblyGoal;
		this.taxTree = taxTreeGoal;
		this.fromGenbank = taxidsFromGenbankGoal;
		this.device = device;
	}

	@Override
	@SuppressWarnings("unchecked")
	protected void doMakeThis() {
		Set<TaxIdNode> wanted = fromGenbank.get();
		if (wanted.isEmpty()) {
			set(Collections.emptyMap());
			return;
		}
		// Optimization of the reference: the assembly summary file is downloaded only if necessary.
		assembly.make();
		List<AssemblyQuality> qualities = (List<AssemblyQuality>) configValue(GSConfigKey.FASTA_QUALITIES);
		int mask = -1;
		if (qualities != null) {
			mask = 0;
			for (AssemblyQuality q : qualities) {
				mask |= 1 << q.ordinal();
			}
		}
		TaxTree tree = taxTree.get();
		File summary = new File(getProject().getCommon().getGenbankDir(), AssemblySummaryReader.ASSEMLY_SUM_GENBANK);
		Map<TaxIdNode, List<AssemblyEntry>> entries = new HashMap<TaxIdNode, List<AssemblyEntry>>();
		try (GpuTaxTree deviceTree = GpuTaxTree.load(device.getAsInt(), getProject().getCommon().getCommonDir(), false)) {
			int[] taxIds = deviceTree.taxIds();
			ByteBuffer filter = ByteBuffer.allocateDirect(Math.max(taxIds.length, 1));
			for (TaxIdNode node : wanted) {
				int i = deviceTree.nodeOf(node.getTaxId());
				if (i >= 0) {
					filter.put(i, (byte) 1);
				}
			}
			try (GpuAssemblySummary picks = GpuAssemblySummary.fromFiles(new String[] { summary.getPath() }, device.getAsInt(),
					deviceTree.taxIdBuffer(), taxIds.length, filter, mask, booleanConfigValue(GSConfigKey.REF_GEN_ONLY), false,
					intConfigValue(GSConfigKey.MAX_FROM_GENBANK))) {
				AssemblyQuality[] byOrdinal = AssemblyQuality.values();
				for (int i = 0; i < picks.picked(); i++) {
					TaxIdNode node = tree.getNodeByTaxId(Integer.toString(taxIds[picks.node(i)]));
					if (node == null) {
						continue;
					}
					List<AssemblyEntry> list = entries.get(node);
					if (list == null) {
						list = new ArrayList<AssemblyEntry>();
						entries.put(node, list);
					}
					list.add(new AssemblyEntry(picks.string(i, 0), picks.string(i, 2), byOrdinal[picks.quality(i)], null, picks.isReference(i),
							picks.string(i, 1)));
				}
				if (getLogger().isTraceEnabled()) {
					getLogger().trace("Entries selected for download: " + picks.picked());
					getLogger().trace("Total number of entries in assembly summary file: " + picks.counted());
				}
			}
		}
		set(entries);
	}
}
