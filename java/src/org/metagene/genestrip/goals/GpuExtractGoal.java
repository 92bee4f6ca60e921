/*
 * The extract goal below the JVM: ExtractGoal.doMakeThis (reference: core/src/main/java/org/metagene/genestrip/goals/
 * ExtractGoal.java:73-129) streams every resource through an AbstractLoggingFastqStreamer and writes the reads whose
 * descriptor starts with extractKey; the override hands the files of each key to gs_host_extract_files
 * (GsGpuNative.hostExtractFiles) in one native call: gzip / BGZF input inflated on the device, the descriptor prefix compared
 * on the device text, the selected records gathered on the device (FASTA input: flagged on the device, written by the host
 * writers) and a .gz output compressed on the device.
 *
 * The reference's path (super.doMakeThis) is kept for everything the native call does not cover:
 *   - writeFilteredFastq off: the goal then writes to standard out;
 *   - a resource that is not a local file (URLs, streams), or whose FASTA type hint disagrees with the suffix rule the
 *     host layer applies to the path (FastqMapGoal.java:64,188-201 -- the same list, so they agree unless a subclass
 *     assigned the hint some other way);
 *   - no key, or a key with a character outside 1..127: ByteArrayUtil.startsWith compares byte != char, so such a key can
 *     match no read; the native call refuses it (GS_E_INVALID).
 * One difference in the file written: under gzipFastqOutput the reference names the file .gz but writes it through a bare
 * FileOutputStream, i.e. uncompressed; the native call writes gzip (BGZF) under a .gz name, the text inside it is the same.
 * SOURCE ONLY (no JDK in the build container); tools/check_java_glue.py checks the reference members used here.
 */
package org.metagene.genestrip.goals;

import java.io.File;
import java.util.ArrayList;
import java.util.LinkedHashMap;
import java.util.List;
import java.util.Map;
import java.util.function.IntSupplier;

import org.metagene.genestrip.ExecutionContext;
import org.metagene.genestrip.GSConfigKey;
import org.metagene.genestrip.GSProject;
import org.metagene.genestrip.GSProject.GSFileType;
import org.metagene.genestrip.fastq.AbstractLoggingFastqStreamer;
import org.metagene.genestrip.gpu.GsGpuNative;
import org.metagene.genestrip.io.StreamingFileResource;
import org.metagene.genestrip.io.StreamingResource;
import org.metagene.genestrip.io.StreamingResourceStream;
import org.metagene.genestrip.make.Goal;
import org.metagene.genestrip.make.ObjectGoal;

public class GpuExtractGoal<P extends GSProject> extends ExtractGoal<P> {
	// FastqMapGoal.java:64 -- the host layer tells FASTA from FASTQ by these suffixes of the path
	private static final String[] FASTA_SUFFIXES = { "fasta", "fa", "fna", "fas", "fasta.gz", "fa.gz", "fna.gz", "fas.gz",
			"fasta.gzip", "fa.gzip", "fna.gzip", "fas.gzip" };

	// (ExtractGoal keeps its own copy private)
	private final ObjectGoal<Map<String, StreamingResourceStream>, P> fastqMap;
	// a supplier, not an int: GSMaker creates its goals inside the superclass constructor, before a subclass's fields are set
	private final IntSupplier device;
	private final long[] totals = new long[4];

	@SafeVarargs
	public GpuExtractGoal(P project, ObjectGoal<Map<String, StreamingResourceStream>, P> fastqMapGoal,
			ExecutionContext bundle, IntSupplier device, Goal<P>... deps) {
		super(project, fastqMapGoal, bundle, deps);
		this.fastqMap = fastqMapGoal;
		this.device = device;
	}

	/** reads / k-mers / base pairs seen and reads written by the last native run of this goal (the sums over its keys) */
	public long[] getTotals() {
		return totals.clone();
	}

	private static boolean isFastaPath(String path) {
		for (String suffix : FASTA_SUFFIXES) {
			if (path.endsWith(suffix)) {
				return true;
			}
		}
		return false;
	}

	private static boolean isDeviceKey(String filter) {
		if (filter == null || filter.isEmpty()) {
			return false;
		}
		for (int i = 0; i < filter.length(); i++) {
			char ch = filter.charAt(i);
			if (ch < 1 || ch > 127) {
				return false;
			}
		}
		return true;
	}

	/** the paths of the resources if every one of them is a local file the host layer reads as the reference would, else null */
	private static String[] localFiles(StreamingResourceStream fastqs) {
		List<String> paths = new ArrayList<>();
		for (StreamingResource r : fastqs) {
			if (!(r instanceof StreamingFileResource)) {
				return null;
			}
			String path = ((StreamingFileResource) r).getFile().getPath();
			if (AbstractLoggingFastqStreamer.FASTA_TYPE_HINT.equals(r.getTypeHint()) != isFastaPath(path)) {
				return null;
			}
			paths.add(path);
		}
		return paths.toArray(new String[0]);
	}

	@Override
	protected void doMakeThis() {
		String filter = stringConfigValue(GSConfigKey.EXTRACT_KEY);
		if (!isDeviceKey(filter) || !booleanConfigValue(GSConfigKey.WRITE_FILTERED_FASTQ)) {
			super.doMakeThis();
			return;
		}
		Map<String, StreamingResourceStream> map = fastqMap.get();
		Map<String, String[]> filesByKey = new LinkedHashMap<>();
		for (String key : map.keySet()) {
			String[] files = localFiles(map.get(key));
			if (files == null) { // one output per key, but one path for the whole goal
				super.doMakeThis();
				return;
			}
			filesByKey.put(key, files);
		}
		int k = intConfigValue(GSConfigKey.KMER_SIZE);
		long[] sum = new long[4];
		for (String key : filesByKey.keySet()) {
			File filteredFile = getProject().getOutputFile(getKey().getName(), key, null, GSFileType.FASTQ_RES,
					booleanConfigValue(GSConfigKey.GZIP_FASTQ_OUTPUT));
			long[] t = new long[4];
			GsGpuNative.hostExtractFiles(device.getAsInt(), filter, k, filesByKey.get(key), filteredFile.getPath(), t);
			for (int i = 0; i < 4; i++) {
				sum[i] += t[i];
			}
		}
		System.arraycopy(sum, 0, totals, 0, 4);
		if (getLogger().isInfoEnabled()) {
			getLogger().info("Extracted " + sum[3] + " of " + sum[0] + " reads on the device.");
		}
	}
}
