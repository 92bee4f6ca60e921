/*
 * The fasta2fastq goal below the JVM: Fasta2FastqGoal.makeFile (reference: core/src/main/java/org/metagene/genestrip/goals/
 * Fasta2FastqGoal.java:92-104) reads the FASTA resources of one key line by line and prints four-line FASTQ with '~'
 * qualities; the override hands their paths to gs_host_fasta2fastq (GsGpuNative.hostFasta2Fastq): records found and rewritten
 * on the device, all files into the one output, gzip under a .gz name as StreamProvider.getOutputStreamForFile gives it.
 * The text is the reference's byte for byte (trailing CR / LF of data lines stripped, empty lines kept as empty data lines,
 * text in front of a first header printed raw); what the device does not take -- a file that does not start with '>', a NUL
 * byte, a record larger than a block -- the host layer's own line-by-line loop writes.  A line of 65 534 bytes or more
 * fails there (IllegalStateException from the native call) as it does in AbstractFastaReader (:104-106).
 *
 * A resource that is not a local file (URLs, streams) keeps the reference's path (super.makeFile).
 * SOURCE ONLY (no JDK in the build container); tools/check_java_glue.py checks the reference members used here.
 */
package org.metagene.genestrip.goals;

import java.io.File;
import java.io.IOException;
import java.util.ArrayList;
import java.util.List;
import java.util.Map;
import java.util.function.IntSupplier;

import org.metagene.genestrip.GSProject;
import org.metagene.genestrip.gpu.GsGpuNative;
import org.metagene.genestrip.io.StreamingFileResource;
import org.metagene.genestrip.io.StreamingResource;
import org.metagene.genestrip.io.StreamingResourceStream;
import org.metagene.genestrip.make.Goal;
import org.metagene.genestrip.make.GoalKey;
import org.metagene.genestrip.make.ObjectGoal;

public class GpuFasta2FastqGoal<P extends GSProject> extends Fasta2FastqGoal<P> {
	// a supplier, not an int: GSMaker creates its goals inside the superclass constructor, before a subclass's fields are set
	private final IntSupplier device;
	private long records;

	@SafeVarargs
	public GpuFasta2FastqGoal(P project, GoalKey key, ObjectGoal<Map<String, StreamingResourceStream>, P> fastaMapGoal,
			IntSupplier device, Goal<P>... deps) {
		super(project, key, fastaMapGoal, deps);
		this.device = device;
	}

	/** records written by the native runs of this goal so far */
	public long getRecords() {
		return records;
	}

	/** the paths of the resources if every one of them is a local file, else null */
	private static String[] localFiles(StreamingResourceStream fastas) {
		List<String> paths = new ArrayList<>();
		for (StreamingResource r : fastas) {
			if (!(r instanceof StreamingFileResource)) {
				return null;
			}
			paths.add(((StreamingFileResource) r).getFile().getPath());
		}
		return paths.toArray(new String[0]);
	}

	@Override
	protected void makeFile(File file) throws IOException {
		String[] files = localFiles(getFastasForFile(file));
		if (files == null) {
			super.makeFile(file);
			return;
		}
		records += GsGpuNative.hostFasta2Fastq(device.getAsInt(), files, file.getPath());
	}
}
