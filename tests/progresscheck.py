"""What tests/test_progress_cpu.py and tests/test_gpu_progress*.py share: a recorder for host.Control and the rules every sequence
of progress records obeys (include/gshost.h, gs_host_control_*)."""
import os
import shutil
import subprocess
import sys

from genestrip_amd import host


class Recorder:
    """callback of a host.Control: keeps every record; stop_at = n: a true answer to the n-th record (1-based)"""

    def __init__(self, stop_at=None):
        self.records, self.stop_at = [], stop_at

    def __call__(self, p):
        self.records.append(p)
        return self.stop_at is not None and len(self.records) == self.stop_at


def run(fn, stop_at=None, every_ms=0):
    """fn() under a Control -> (result or None, Cancelled or None, records)"""
    rec = Recorder(stop_at)
    with host.Control(rec, every_ms=every_ms):
        try:
            return fn(), None, rec.records
        except host.Cancelled as e:
            assert e.code == -8
            return None, e, rec.records


def check_records(records, paths, complete):
    """the rules of a sequence of records over the files `paths`; complete: the call ran to its end (else: it was stopped, and the
    last record is the record of the stop).  -> {file: file_reads of its last record}"""
    sizes = [os.path.getsize(p) for p in paths]
    assert records, "no record at all"
    seen, closed, last_done = {}, set(), 0
    for i, r in enumerate(records):
        assert r.n_files == len(paths) and r.total_bytes_total == sum(sizes), r
        assert 0 <= r.file < len(paths) and r.file_bytes_total == sizes[r.file], r
        closing = i == len(records) - 1 and r.file in closed and r.file_done == 1 and r.files_done == len(paths)
        assert closing or not (complete and i == len(records) - 1), ("no closing record", r)
        if r.file not in seen:
            assert r.file_bytes_done == 0 and r.file_done == 0 and r.file_reads == 0, ("first record of a file", r)
        else:
            assert r.file_bytes_done >= seen[r.file].file_bytes_done, ("bytes went back", seen[r.file], r)
        assert 0 <= r.file_bytes_done <= r.file_bytes_total, r
        assert r.files_done >= last_done and r.files_done == len(closed) + (1 if r.file_done and not closing else 0), r
        assert r.seconds_file >= 0 and r.seconds_total >= 0
        if not closing:
            assert r.file not in closed, ("a record behind the file's last", r)
            if r.file_done:
                assert r.file_bytes_done == r.file_bytes_total, r
                closed.add(r.file)
        last_done = r.files_done
        seen[r.file] = r
        assert r.total_bytes_done == sum(x.file_bytes_done for x in seen.values()), r
        assert r.total_reads == sum(x.file_reads for x in seen.values()), r
    if complete:
        assert len(closed) == len(paths) and records[-1].files_done == len(paths) and records[-1].file_done == 1
        assert records[-1].total_bytes_done == sum(sizes)
    return {f: r.file_reads for f, r in seen.items()}


# ---- the Java side (java/src/.../gpu/GpuProgress.java and its two callers) through tools/check_java_glue.py.  No JDK and no
# reference checkout where the suite runs, so the checker gets a stand-in library: declarations only, with the names, arities and
# visibilities of the reference's members that the progress glue uses (ExecutionContext.java:88-110, fastq/
# FastqReaderInterruptedException.java, io/StreamingResource.java).
JAVA_LIBRARY = {
    "core/src/main/java/org/metagene/genestrip/ExecutionContext.java": """package org.metagene.genestrip;
import org.metagene.genestrip.io.StreamingResource;
public interface ExecutionContext {
	public void setTotalProgress(long a, long b, long c, long d, double e, long f, int g, int h);
	public void setFastqProgress(StreamingResource r, long a, long b, long c, long d, double e, long f);
	public boolean isRequiresProgress();
}
""",
    "core/src/main/java/org/metagene/genestrip/fastq/FastqReaderInterruptedException.java": """package org.metagene.genestrip.fastq;
public class FastqReaderInterruptedException extends RuntimeException {
	public FastqReaderInterruptedException() {
	}
}
""",
    "core/src/main/java/org/metagene/genestrip/io/StreamingResource.java": """package org.metagene.genestrip.io;
public interface StreamingResource {
	public String getName();
}
""",
}


def check_progress_glue(tmp_path, edit=None):
    """tools/check_java_glue.py over GpuProgress.java and GsGpuNative.java against the stand-in library -> (exit code, output);
    edit: a function on the source of GpuProgress.java (to show that the checker looks)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref, glue = tmp_path / "ref", tmp_path / "glue" / "org" / "metagene" / "genestrip" / "gpu"
    for rel, text in JAVA_LIBRARY.items():
        (ref / rel).parent.mkdir(parents=True, exist_ok=True)
        (ref / rel).write_text(text)
    glue.mkdir(parents=True, exist_ok=True)
    src = os.path.join(root, "java", "src", "org", "metagene", "genestrip", "gpu")
    shutil.copy(os.path.join(src, "GsGpuNative.java"), glue / "GsGpuNative.java")
    text = open(os.path.join(src, "GpuProgress.java")).read()
    (glue / "GpuProgress.java").write_text(edit(text) if edit else text)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_java_glue.py"), "--reference", str(ref), "--glue", str(tmp_path / "glue")],
                       capture_output=True, text=True)
    return r.returncode, r.stdout
