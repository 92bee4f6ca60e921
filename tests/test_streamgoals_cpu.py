"""extract and fasta2fastq without a device: the helper (tests/streamgoals.py, the two Java loops restated) against hand-written
cases, and the host layer's reference-exact path (GS_HOST_FAST=0 -- host code only) against the helper on the same cases."""
import gzip
import os
import re
import subprocess
import sys

import pytest

import genestrip_amd as ga
import streamgoals as sg
from conftest import GOLDEN, ROOT
from genestrip_amd import host

FIXTURE = os.path.join(GOLDEN, "fasta2fastq", "fasta2fastqtest.fasta")

# (input, what the goal prints) -- by hand from Fasta2FastqGoal.java:133-164
F2F_CASES = {
    "crlf, \\r\\r\\n and empty lines": (b">h1 x\r\nACGT\r\nAC\r\r\n\nGG\n\r\n>h2\nT\n", b"@h1 x\r\nACGTACGG\n+\n~~~~~~~~\n@h2\nT\n+\n~\n"),
    "a record without data": (b">a\n>b\nAC\n>c\n", b"@a\n\n+\n\n@b\nAC\n+\n~~\n@c\n\n+\n\n"),
    "text before the first header": (b"junk\r\nmore\n>h\nAC\n", b"junkmore@h\nAC\n+\n~~\n"),
    "a last header without newline": (b">a\nAC\n>last", b"@a\nAC\n+\n~~\n@las\n\n+\n\n"),
    "a last data line without newline": (b">a\nAC\nGT\r", b"@a\nACGT\n+\n~~~~\n"),
    "a NUL inside a line": (b">a\0b\nA\0C\n\0\n", b"@ab\nAC\n+\n~~\n"),
    "no header at all": (b"AC\nGT\n", b"ACGT"),
    "empty": (b"", b""),
    "a byte >= 0x80": (b">h\xc3\nA\xa9\n", b"@h\xef\xbf\x83\nA\xef\xbe\xa9\n+\n~~\n"),
}

FASTQ = (b"@abc\nACGT\n+\nIIII\n" b"@abc\r\nAC\r\n+\r\nII\r\n" b"@\nGG\n+\nII\n" b"@abcd e\nTTT\n+abcd\nJJJ\n" b"@xabc\nA\n+\nI\n")
# key -> records selected (ExtractGoal.java:93: the descriptor behind its first byte starts with the key)
EXTRACT_KEYS = {b"a": [0, 1, 3], b"abc": [0, 1, 3], b"abcd": [3], b"abc\r": [1], b"abcd e": [3], b"abcd ef": [], b"x": [4], b"@": []}


@pytest.mark.parametrize("name", sorted(F2F_CASES))
def test_helper_fasta2fastq_by_hand(name):
    data, want = F2F_CASES[name]
    assert sg.fasta2fastq(data)[0] == want


def test_helper_line_length_limit():
    assert sg.fasta2fastq(b">a\n" + b"A" * 65532 + b"\n")[0].endswith(b"~\n")
    with pytest.raises(sg.LineTooLong):
        sg.fasta2fastq(b">a\n" + b"A" * 65533 + b"\n")  # 65 534 bytes with the newline


def test_helper_extract_by_hand():
    recs = [b"@abc\nACGT\n+\nIIII\n", b"@abc\r\nAC\r\n+\nII\r\n", b"@\nGG\n+\nII\n", b"@abcd e\nTTT\n+\nJJJ\n", b"@xabc\nA\n+\nI\n"]
    for key, sel in EXTRACT_KEYS.items():
        assert sg.extract(FASTQ, key) == (b"".join(recs[i] for i in sel), len(sel)), key
    fa = b">s1 a\nAC\r\nGT\n>s2\nTT\n"
    assert sg.extract(fa, b"s", fasta=True) == (b"@s1 a\nAC\rGT\n+\n~~~~~\n@s2\nTT\n+\n~~\n", 2)
    assert sg.extract(fa, b"s1 a", fasta=True)[1] == 1 and sg.extract(fa, b"s1 ab", fasta=True)[1] == 0


def test_fixture_goal_output_equals_reader_and_write():
    """T/goals/Fasta2FastqGoalTest.java:67-80: on the reference's own test input the goal's output equals the FASTA-mode reader's
    records written as ReadEntry.write"""
    data = open(FIXTURE, "rb").read()
    assert len(data) == 9175 and b"\r" not in data
    out, n = sg.fasta2fastq(data)
    assert n == 6
    rd = host.FastqReader(FIXTURE, k=31, fasta=True)
    want = bytearray()
    b = rd.next_batch()
    assert b["n_reads"] == 6
    for i in range(6):
        desc = bytes(b["desc"][int(b["desc_off"][i]):int(b["desc_off"][i + 1])])
        seq = bytes(b["seq"][int(b["seq_off"][i]):int(b["seq_off"][i + 1])])
        want += desc + b"\n" + seq + b"\n+\n" + b"~" * len(seq) + b"\n"
    rd.close()
    assert out == bytes(want)


@pytest.fixture()
def cpu_path(monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")


@pytest.mark.parametrize("name", sorted(F2F_CASES))
def test_library_cpu_path_fasta2fastq(name, tmp_path, cpu_path):
    data, _ = F2F_CASES[name]
    src, dst = tmp_path / "in.fasta", tmp_path / "out.fastq"
    src.write_bytes(data)
    want, n = sg.fasta2fastq(data)
    assert host.fasta2fastq([src], dst) == n
    assert dst.read_bytes() == want


def test_library_cpu_path_fasta2fastq_files_and_gzip(tmp_path, cpu_path):
    a, b = open(FIXTURE, "rb").read(), F2F_CASES["crlf, \\r\\r\\n and empty lines"][0]
    (tmp_path / "a.fa.gz").write_bytes(gzip.compress(a))
    (tmp_path / "b.fa").write_bytes(b)
    dst = tmp_path / "out.fastq.gz"
    assert host.fasta2fastq([tmp_path / "a.fa.gz", tmp_path / "b.fa"], dst) == 8
    assert gzip.decompress(dst.read_bytes()) == sg.fasta2fastq_files([a, b])


def test_library_cpu_path_line_length_limit(tmp_path, cpu_path):
    src, dst = tmp_path / "in.fasta", tmp_path / "out.fastq"
    src.write_bytes(b">a\n" + b"A" * 65532 + b"\n")
    assert host.fasta2fastq([src], dst) == 1
    src.write_bytes(b">a\n" + b"A" * 65533 + b"\n")
    with pytest.raises(ga.GsError) as e:
        host.fasta2fastq([src], dst)
    assert e.value.code == -1


@pytest.mark.parametrize("key", sorted(EXTRACT_KEYS))
def test_library_cpu_path_extract(key, tmp_path, cpu_path):
    src, dst = tmp_path / "in.fastq", tmp_path / "out.fastq"
    src.write_bytes(FASTQ)
    want, n = sg.extract(FASTQ, key)
    tot = host.extract_files(key, [src], dst, k=3)
    assert dst.read_bytes() == want
    assert (tot.filtered_reads, tot.reads, tot.bps, tot.kmers) == (n, 5, 4 + 3 + 2 + 3 + 1, 2 + 1 + 0 + 1 + 0)


def test_library_cpu_path_extract_fasta_and_two_files(tmp_path, cpu_path):
    fa = b">s1 a\nAC\r\nGT\n>t2\nTT\n>s3\n"
    (tmp_path / "a.fasta").write_bytes(fa)
    (tmp_path / "b.fastq.gz").write_bytes(gzip.compress(FASTQ))
    dst = tmp_path / "out.fastq.gz"
    tot = host.extract_files(b"s", [tmp_path / "a.fasta", tmp_path / "b.fastq.gz"], dst)
    assert gzip.decompress(dst.read_bytes()) == sg.extract(fa, b"s", fasta=True)[0] + sg.extract(FASTQ, b"s")[0]
    assert (tot.filtered_reads, tot.reads) == (2, 8)


def test_invalid_keys(tmp_path, cpu_path):
    src = tmp_path / "in.fastq"
    src.write_bytes(FASTQ)
    for key in (b"", b"ab\xc3", b"\x80"):
        with pytest.raises(ga.GsError) as e:
            host.extract_files(key, [src], tmp_path / "out.fastq")
        assert e.value.code == -1


# ---- the Java goal classes (java/src) through tools/check_java_glue.py, as tests/test_java_glue_cpu.py does for the others.
# No JDK and no reference checkout where the suite runs, so the checker gets a stand-in library: declarations only, with the
# names, arities and visibilities of the members GpuExtractGoal and GpuFasta2FastqGoal rely on.
GLUE_SRC = os.path.join(ROOT, "java", "src", "org", "metagene", "genestrip")
GLUE_LIBRARY = {
    "base/src/main/java/org/metagene/genestrip/make/Goal.java": '''
package org.metagene.genestrip.make;
public abstract class Goal<P extends Project> {
	public Goal(P project, GoalKey goalKey, Goal<P>... dependencies) { }
	public P getProject() { return null; }
	public GoalKey getKey() { return null; }
	protected org.apache.commons.logging.Log getLogger() { return null; }
	public final void make() { }
	protected void doMakeThis() { }
	protected int intConfigValue(ConfigKey key) { return 0; }
	protected boolean booleanConfigValue(ConfigKey key) { return false; }
	protected String stringConfigValue(ConfigKey key) { return null; }
}
''',
    "base/src/main/java/org/metagene/genestrip/make/ObjectGoal.java": '''
package org.metagene.genestrip.make;
public abstract class ObjectGoal<T, P extends Project> extends Goal<P> {
	public ObjectGoal(P project, GoalKey key, Goal<P>... deps) { super(project, key, deps); }
	public final T get() { return null; }
}
''',
    "base/src/main/java/org/metagene/genestrip/make/FileListGoal.java": '''
package org.metagene.genestrip.make;
import java.io.File;
import java.io.IOException;
import java.util.List;
public abstract class FileListGoal<P extends Project> extends Goal<P> {
	public FileListGoal(P project, GoalKey key, List<File> files, Goal<P>... deps) { super(project, key, deps); }
	protected abstract void makeFile(File file) throws IOException;
}
''',
    "base/src/main/java/org/metagene/genestrip/make/GoalKey.java": '''
package org.metagene.genestrip.make;
public interface GoalKey {
	String getName();
}
''',
    "base/src/main/java/org/metagene/genestrip/io/StreamingResource.java": '''
package org.metagene.genestrip.io;
public interface StreamingResource {
	String getName();
	default String getTypeHint() { return null; }
}
''',
    "base/src/main/java/org/metagene/genestrip/io/StreamingFileResource.java": '''
package org.metagene.genestrip.io;
import java.io.File;
public class StreamingFileResource implements StreamingResource {
	private final File file;
	public StreamingFileResource(File file) { this.file = file; }
	public String getName() { return null; }
	public File getFile() { return file; }
}
''',
    "base/src/main/java/org/metagene/genestrip/io/StreamingResourceStream.java": '''
package org.metagene.genestrip.io;
public interface StreamingResourceStream extends Iterable<StreamingResource> {
	int size();
}
''',
    "core/src/main/java/org/metagene/genestrip/ExecutionContext.java": '''
package org.metagene.genestrip;
public interface ExecutionContext {
	int getThreads();
}
''',
    "core/src/main/java/org/metagene/genestrip/GSConfigKey.java": '''
package org.metagene.genestrip;
public enum GSConfigKey {
	KMER_SIZE, EXTRACT_KEY, GZIP_FASTQ_OUTPUT, WRITE_FILTERED_FASTQ;
}
''',
    "core/src/main/java/org/metagene/genestrip/GSProject.java": '''
package org.metagene.genestrip;
import java.io.File;
public class GSProject {
	public enum GSFileType {
		FASTQ, FASTQ_RES;
	}
	public File getOutputFile(String goal, String key, String name, GSFileType type, boolean gzip) { return null; }
}
''',
    "core/src/main/java/org/metagene/genestrip/fastq/AbstractLoggingFastqStreamer.java": '''
package org.metagene.genestrip.fastq;
public abstract class AbstractLoggingFastqStreamer {
	public static final String FASTA_TYPE_HINT = "fasta";
}
''',
    "core/src/main/java/org/metagene/genestrip/goals/ExtractGoal.java": '''
package org.metagene.genestrip.goals;
import java.util.Map;
import org.metagene.genestrip.ExecutionContext;
import org.metagene.genestrip.GSProject;
import org.metagene.genestrip.io.StreamingResourceStream;
import org.metagene.genestrip.make.Goal;
import org.metagene.genestrip.make.ObjectGoal;
public class ExtractGoal<P extends GSProject> extends Goal<P> {
	private final ObjectGoal<Map<String, StreamingResourceStream>, P> fastqMapGoal;
	private final ExecutionContext bundle;
	public ExtractGoal(P project, ObjectGoal<Map<String, StreamingResourceStream>, P> fastqMapGoal, ExecutionContext bundle, Goal<P>... deps) {
		super(project, null, deps);
	}
	@Override
	protected void doMakeThis() { }
}
''',
    "core/src/main/java/org/metagene/genestrip/goals/Fasta2FastqGoal.java": '''
package org.metagene.genestrip.goals;
import java.io.File;
import java.io.IOException;
import java.util.Map;
import org.metagene.genestrip.GSProject;
import org.metagene.genestrip.io.StreamingResourceStream;
import org.metagene.genestrip.make.FileListGoal;
import org.metagene.genestrip.make.Goal;
import org.metagene.genestrip.make.GoalKey;
import org.metagene.genestrip.make.ObjectGoal;
public class Fasta2FastqGoal<P extends GSProject> extends FileListGoal<P> {
	private final ObjectGoal<Map<String, StreamingResourceStream>, P> fastaMapGoal;
	public Fasta2FastqGoal(P project, GoalKey key, ObjectGoal<Map<String, StreamingResourceStream>, P> fastaMapGoal, Goal<P>... deps) {
		super(project, key, null, deps);
	}
	protected StreamingResourceStream getFastasForFile(File file) { return null; }
	@Override
	protected void makeFile(File file) throws IOException { }
}
''',
}
GLUE_CLASSES = ("goals/GpuExtractGoal.java", "goals/GpuFasta2FastqGoal.java", "gpu/GsGpuNative.java")


def _check_glue(tmp_path, name, edit=None):
    ref = tmp_path / "ref"
    for rel, text in GLUE_LIBRARY.items():
        (ref / rel).parent.mkdir(parents=True, exist_ok=True)
        (ref / rel).write_text(text)
    glue = tmp_path / name
    for rel in GLUE_CLASSES:
        dst = glue / "org" / "metagene" / "genestrip" / rel
        dst.parent.mkdir(parents=True, exist_ok=True)
        text = open(os.path.join(GLUE_SRC, rel)).read()
        dst.write_text(edit(rel, text) if edit else text)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_java_glue.py"), "--reference", str(ref), "--glue", str(glue)],
                       capture_output=True, text=True)
    return r.returncode, r.stdout


def test_java_goal_classes_pass_the_glue_check(tmp_path):
    rc, out = _check_glue(tmp_path, "glue")
    assert rc == 0, out
    assert "checked %d glue classes against %d reference files: 0 finding(s)" % (len(GLUE_CLASSES), len(GLUE_LIBRARY)) in out, out

    # the check has teeth on exactly these classes: a misspelt hook, a native called with one argument too few, a private
    # field of the superclass and an override of a final method are each reported
    def broken(rel, text):
        if rel.endswith("GpuFasta2FastqGoal.java"):
            text = text.replace("getFastasForFile(file)", "getFastaForFile(file)").replace("protected void makeFile(File file)", "public void make()")
        if rel.endswith("GpuExtractGoal.java"):
            text = text.replace("filteredFile.getPath(), t);", "t);").replace("fastqMap.get()", "fastqMapGoal.get()")
        return text
    rc, out = _check_glue(tmp_path, "broken", broken)
    assert rc == 1
    for needle in ("getFastaForFile", "@Override make", "is final", "hostExtractFiles(...): no overload takes 5", "fastqMapGoal"):
        assert needle in out, (needle, out)


def test_java_goal_classes_are_wired_and_fall_back():
    src = {n: open(os.path.join(GLUE_SRC, *n.split("/"))).read() for n in GLUE_CLASSES + ("GpuGSMaker.java",)}
    natives = src["gpu/GsGpuNative.java"]
    assert re.search(r"static\s+native\s+void\s+hostExtractFiles\(", natives) and re.search(r"static\s+native\s+long\s+hostFasta2Fastq\(", natives)
    ex, f2f, maker = src["goals/GpuExtractGoal.java"], src["goals/GpuFasta2FastqGoal.java"], src["GpuGSMaker.java"]
    assert "extends ExtractGoal<P>" in ex and "protected void doMakeThis()" in ex and "GsGpuNative.hostExtractFiles(" in ex
    # the reference's path for what the native call does not cover: standard out, a resource that is not a local file
    assert ex.count("super.doMakeThis();") >= 2 and "GSConfigKey.WRITE_FILTERED_FASTQ" in ex and "instanceof StreamingFileResource" in ex
    assert "extends Fasta2FastqGoal<P>" in f2f and "protected void makeFile(File file)" in f2f and "GsGpuNative.hostFasta2Fastq(" in f2f
    assert "super.makeFile(file);" in f2f and "instanceof StreamingFileResource" in f2f
    assert "protected void registerGoal(Goal<P> goal)" in maker and "new GpuExtractGoal<P>(" in maker and "new GpuFasta2FastqGoal<P>(" in maker
