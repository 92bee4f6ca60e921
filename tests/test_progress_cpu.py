"""Progress and cancellation of the file-level calls without a device: the control handle of include/gshost.h, its C++ core
(genestrip_amd/csrc/gs_control.h) under the sanitizers, and the extract / fasta2fastq goals on the host layer's reference-exact path
(GS_HOST_FAST=0 -- host code only) with a control attached: the records obey the rules, a run that is not stopped writes the bytes it
writes without a control, a run stopped at its n-th record leaves the output of exactly the records its last record reports."""
import ctypes as C
import os
import shutil
import subprocess
import threading

import pytest

import genestrip_amd as ga
import streamgoals as sg
from genestrip_amd import binding, host
from progresscheck import check_progress_glue, check_records, run

HERE = os.path.dirname(os.path.abspath(__file__))


def test_symbols_and_status_text():
    L = host.lib()
    for name in ("create", "destroy", "cancel", "snapshot", "attach"):
        assert hasattr(L, "gs_host_control_" + name)
    assert binding.lib().gs_strerror(-8).decode() == "cancelled"
    assert binding.lib().gs_abi_version() == 3
    assert issubclass(host.Cancelled, ga.GsError) and host.Cancelled(x=1).code == -8 and host.Cancelled(x=1).x == 1


def test_handle_life_cycle():
    L = host.lib()
    h = C.c_void_p()
    assert L.gs_host_control_create(C.byref(h), None, None, 0) == 0 and h.value
    p, flag = host.Progress(), C.c_int32(7)
    assert L.gs_host_control_snapshot(h, C.byref(p), C.byref(flag)) == 0
    assert flag.value == 0 and (p.n_files, p.total_reads, p.file_bytes_done) == (0, 0, 0)
    assert L.gs_host_control_attach(h) == 0 and L.gs_host_control_attach(None) == 0
    assert L.gs_host_control_cancel(h) == 0
    assert L.gs_host_control_snapshot(h, C.byref(p), C.byref(flag)) == 0 and flag.value == 1
    assert L.gs_host_control_snapshot(h, None, None) == -1
    assert L.gs_host_control_destroy(h) == 0
    # a destroyed handle and NULL: GS_E_INVALID from every call
    for bad in (h, None):
        assert L.gs_host_control_destroy(bad) == -1
        assert L.gs_host_control_cancel(bad) == -1
        assert L.gs_host_control_snapshot(bad, C.byref(p), C.byref(flag)) == -1
    assert L.gs_host_control_attach(h) == -1
    assert b"control" in L.gs_host_last_error()
    assert L.gs_host_control_create(None, None, None, 0) == -1


def test_control_object_without_a_call():
    with host.Control() as ctl:
        p, stop = ctl.snapshot()
        assert not stop and p.n_files == 0
        t = threading.Thread(target=ctl.cancel)  # (any thread)
        t.start()
        t.join()
        assert ctl.snapshot()[1]
    assert ctl.h is None


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_control_under_sanitizers(tmp_path, sanitizer):
    """gs_control.h alone (tests/native/control_sanitize.cpp): a publisher, two readers of snapshots, a canceller"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(HERE, "native", "control_sanitize.cpp")
    exe = str(tmp_path / "control_sanitize")
    flags = ["-O1", "-g", f"-fsanitize={sanitizer}", "-std=c++17", "-pthread"]
    b = subprocess.run(["g++", *flags, "-o", exe, src], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


# ---- the two goals on the host-only path, batches of 3 records (GS_HOST_BATCH_READS), two files each
def _fastq(n, tag):
    return b"".join(b"@%s%d x\n%s\n+\n%s\n" % (tag, i, b"ACGT" * (i % 5 + 1), b"IJKL" * (i % 5 + 1)) for i in range(n))


def _fasta(n, tag):
    return b"".join(b">%s%d y\n%s\n%s\n" % (tag, i, b"ACGTT" * (i % 4 + 1), b"GG" * (i % 3)) for i in range(n))


def _fastq_prefix(data, n):
    return b"".join(data.splitlines(keepends=True)[:4 * n])


def _fasta_prefix(data, n):
    out, seen = [], 0
    for ln in data.splitlines(keepends=True):
        seen += ln.startswith(b">")
        if seen > n:
            break
        out.append(ln)
    return b"".join(out)


@pytest.fixture()
def cpu_path(monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    monkeypatch.setenv("GS_HOST_BATCH_READS", "3")


EXTRACT_IN = [("a.fastq", _fastq(10, b"ab")), ("b.fastq", _fastq(7, b"ac") + _fastq(4, b"ab"))]
F2F_IN = [("a.fasta", _fasta(10, b"s")), ("b.fasta", _fasta(8, b"t"))]


def _write(tmp_path, files):
    paths = []
    for name, data in files:
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    return paths


def _extract_case(tmp_path):
    paths = _write(tmp_path, EXTRACT_IN)
    dst = tmp_path / "out.fastq"
    return paths, dst, (lambda: host.extract_files(b"ab", paths, dst, k=3)), (lambda d, n: sg.extract(_fastq_prefix(d, n), b"ab")[0])


def _f2f_case(tmp_path):
    paths = _write(tmp_path, F2F_IN)
    dst = tmp_path / "out.fastq"
    return paths, dst, (lambda: host.fasta2fastq(paths, dst)), (lambda d, n: sg.fasta2fastq(_fasta_prefix(d, n))[0])


CASES = {"extract": (_extract_case, EXTRACT_IN), "fasta2fastq": (_f2f_case, F2F_IN)}


@pytest.mark.parametrize("goal", sorted(CASES))
def test_records_and_output_of_a_whole_run(goal, tmp_path, cpu_path):
    make, files = CASES[goal]
    paths, dst, call, want = make(tmp_path)
    plain = call()
    plain_bytes = dst.read_bytes()
    got, stop, records = run(call)
    assert stop is None and dst.read_bytes() == plain_bytes == b"".join(want(d, 10 ** 6) for _, d in files)
    reads = check_records(records, paths, complete=True)
    n_in = [len(files[0][1].split(b"\n@" if goal == "extract" else b"\n>")), len(files[1][1].split(b"\n@" if goal == "extract" else b"\n>"))]
    assert [reads[0], reads[1]] == n_in
    if goal == "extract":
        assert (got.reads, got.filtered_reads) == (plain.reads, plain.filtered_reads) == (sum(n_in), 14)
        assert records[-1].total_reads == got.reads
    else:
        assert got == plain == sum(n_in) == records[-1].total_reads
    # more than a start and an end per file: the batches report as well, and every_ms = 0 shows all of them
    assert len(records) >= 2 * (1 + 2 + 1) + 1
    # an interval nobody reaches: only the first and last record of each file and the closing one come through
    _, _, sparse = run(call, every_ms=3600000)
    assert [(r.file, r.file_done) for r in sparse] == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 1)]
    assert dst.read_bytes() == plain_bytes


@pytest.mark.parametrize("goal", sorted(CASES))
def test_stop_at_every_record(goal, tmp_path, cpu_path):
    make, files = CASES[goal]
    paths, dst, call, want = make(tmp_path)
    _, _, all_records = run(call)
    for n in range(1, len(all_records) + 1):  # the first, every one in the middle, the last chunk record, the closing one
        got, stop, records = run(call, stop_at=n)
        assert got is None and stop is not None, n
        at_end = all_records[n - 1].file_done == 1  # (the answer to a file's last record or to the closing one: that record stands)
        assert len(records) == (n if at_end else n + 1), n  # the record of the stop follows, unless nothing was left to count
        reads = check_records(records, paths, complete=False)
        per_file = [reads.get(0, 0), reads.get(1, 0)]
        assert dst.read_bytes() == b"".join(want(d, per_file[f]) for f, (_, d) in enumerate(files)), (n, per_file)
        if goal == "extract":
            assert stop.totals.reads == sum(per_file) == records[-1].total_reads
            assert stop.totals.filtered_reads == dst.read_bytes().count(b"\n+\n")
        else:
            assert stop.records == sum(per_file)
    assert sum(per_file) == all_records[-1].total_reads  # (the stop at the closing record came behind everything)


def test_cancel_flag_set_beforehand_and_callback_exception(tmp_path, cpu_path):
    paths, dst, call, want = _extract_case(tmp_path)
    with host.Control() as ctl:  # no callback: the flag alone, looked at with the first record
        ctl.cancel()
        with pytest.raises(host.Cancelled) as e:
            call()
        assert e.value.totals.reads == 0 and dst.read_bytes() == b""
        p, stop = ctl.snapshot()
        assert stop and (p.file, p.file_reads, p.n_files) == (0, 0, 2)

    def boom(p):
        raise KeyError("from the callback")
    with pytest.raises(KeyError):
        with host.Control(boom):
            call()
    assert call().reads == 21  # the thread is detached again: as before


def test_java_progress_glue(tmp_path):
    """GpuProgress.java against a stand-in for the reference's declarations (tests/progresscheck.py); a misspelt member is found"""
    rc, out = check_progress_glue(tmp_path / "good")
    assert rc == 0 and "checked 2 glue classes" in out and "0 finding(s)" in out, out
    rc, out = check_progress_glue(tmp_path / "bad", lambda src: src.replace("bundle.setTotalProgress(", "bundle.setTotalProgres(", 1))
    assert rc == 1 and "setTotalProgres" in out, out


def test_gz_output_of_the_line_loop_is_byte_equal_under_a_control(tmp_path, cpu_path, monkeypatch):
    """fasta2fastq's line loop reports every fifty records here; the .gz output -- packed buffer by buffer on the writer's thread --
    keeps its member boundaries: a control that is not cancelled changes no byte"""
    monkeypatch.setenv("GS_HOST_BATCH_READS", "50")
    data = _fasta(9000, b"s") * 16  # (megabytes of output: the loop hands several buffers to the writer, which packs them one by one)
    src, dst = tmp_path / "big.fasta", tmp_path / "out.fastq.gz"
    src.write_bytes(data)
    call = lambda: host.fasta2fastq([str(src)], dst)
    n = call()
    raw = dst.read_bytes()
    got, stop, records = run(call)
    assert stop is None and got == n == 144000 and len(records) > 1000
    assert dst.read_bytes() == raw and len(raw) > 100000
    import gzip
    assert gzip.decompress(raw) == sg.fasta2fastq(data)[0] and len(gzip.decompress(raw)) > (5 << 20)


def test_a_control_inside_another_gives_the_thread_back(tmp_path, cpu_path):
    paths, dst, call, want = _extract_case(tmp_path)
    outer, inner = [], []
    with host.Control(lambda p: outer.append(p)):
        with host.Control(lambda p: inner.append(p)):
            call()
        n_inner = len(inner)
        assert n_inner > 0 and not outer
        call()  # the outer control is this thread's again
        assert len(outer) == n_inner and len(inner) == n_inner
    call()
    assert len(outer) == n_inner
