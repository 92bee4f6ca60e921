"""Progress and cancellation through the JNI shim (java/jni/gsgpu_jni.c against the stand-in JNIEnv, built as tests/test_gpu_jni.py
builds it): hostControlSnapshot fills its array, hostControlCancel from a second thread ends hostMatchRun with the exception the
Java side turns into FastqReaderInterruptedException, and the matcher's run finishes to the reference's table over exactly the reads
the last snapshot reports.  The Java sources that poll the control are checked statically (tools/check_java_glue.py)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
from conftest import ROOT
from genestrip_amd import synth
from oracle import gs_oracle as orc
from progresscheck import check_progress_glue
from test_gpu_jni import PFX, _buf, _str, _strings, jni  # noqa: F401 -- the fixture and the helpers, as they are

pytestmark = pytest.mark.gpu

N = 20000


def _natives(L):
    vp, i64 = C.c_void_p, C.c_int64
    for name, res, args in (("hostControlCreate", i64, [vp, vp]), ("hostControlDestroy", None, [vp, vp, i64]), ("hostControlCancel", None, [vp, vp, i64]),
                            ("hostControlAttach", None, [vp, vp, i64]), ("hostControlSnapshot", None, [vp, vp, i64, vp])):
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, args
    return lambda name, *a: getattr(L, PFX + name)(L.stub_env(), None, *a)


def _snapshot(L, call, h):
    arr = L.stub_long_array(13)
    call("hostControlSnapshot", h, arr)
    return [L.stub_long_array_get(arr, i) for i in range(13)]


def test_control_natives(jni):
    L = jni
    call = _natives(L)
    h = call("hostControlCreate")
    assert h and L.stub_take_exception() is None
    assert _snapshot(L, call, h) == [0] * 13
    call("hostControlAttach", h)
    call("hostControlAttach", 0)
    call("hostControlCancel", h)
    assert L.stub_take_exception() is None and _snapshot(L, call, h)[12] == 1
    call("hostControlSnapshot", h, L.stub_long_array(5))  # too short an array
    assert b"gsgpu error -1" in L.stub_take_exception()
    call("hostControlDestroy", h)
    assert L.stub_take_exception() is None
    for name in ("hostControlDestroy", "hostControlCancel", "hostControlAttach"):  # a destroyed handle
        call(name, h)
        assert b"gsgpu error -1" in L.stub_take_exception(), name


def test_cancel_from_a_second_thread_ends_host_match_run(jni, tmp_path, monkeypatch):
    L = jni
    call = _natives(L)
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    sdb = synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)
    seq, off = synth.reads_host(sdb.genomes, N, read_len=150, seed=31)
    reads = [seq[int(off[i]):int(off[i + 1])].tobytes() for i in range(N)]
    path = str(tmp_path / "in.fastq")
    open(path, "wb").write(b"".join(b"@read%d l=%d\n%s\n+\n%s\n" % (i, i % 5, s, b"F" * len(s)) for i, s in enumerate(reads)))
    store = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    m = ga.FastqKMerMatcher(store)
    h = call("hostControlCreate")
    call("hostControlAttach", h)  # (this thread makes the call)
    env, snap_fn, cancel_fn, arr = L.stub_env(), getattr(L, PFX + "hostControlSnapshot"), getattr(L, PFX + "hostControlCancel"), L.stub_long_array(13)

    def canceller():  # as the Java daemon thread: polls, and cancels as soon as the call has reported its first chunk
        while True:
            snap_fn(env, None, h, arr)
            if L.stub_long_array_get(arr, 4) > 0 or L.stub_long_array_get(arr, 3) > 0:
                break
        cancel_fn(env, None, h)

    t = threading.Thread(target=canceller)
    t.start()
    totals = L.stub_long_array(4)
    descs = np.zeros((sdb.n_values, 256), dtype=np.uint8)
    kr = str(tmp_path / "kr.txt")
    getattr(L, PFX + "hostMatchRun")(env, None, m.h.value, store.h.value, _strings(L, [path]), None, _str(L, kr), 1, _strings(L, sdb.taxids), 0,
                                     _buf(L, descs), 256, totals)
    t.join()
    exc = L.stub_take_exception()
    call("hostControlAttach", 0)
    snap = _snapshot(L, call, h)
    call("hostControlDestroy", h)
    assert exc is not None and exc.startswith(b"cancelled"), exc
    n = snap[6]
    assert snap[12] == 1 and snap[1] == 1 and 0 < n < N and snap[9] == n
    assert [L.stub_long_array_get(totals, i) for i in range(3)] == [n, n * 120, n * 150]  # (filled in front of the throw)
    table, dtable = m.finish()
    odb = orc.DB(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    o = matchcheck.oracle_batch(odb, np.frombuffer(b"".join(reads[:n]), dtype=np.uint8), np.arange(n + 1, dtype=np.uint64) * 150)
    matchcheck.check_match(o, dict(table=table, dtable=dtable), "hostMatchRun, cancelled")
    assert open(kr, "rb").read().count(b"\n") == n
    m.close()
    store.close()


def test_java_glue_still_passes(tmp_path):
    """the Java side of the control -- GpuProgress and the natives it calls -- under tools/check_java_glue.py (a stand-in library:
    tests/progresscheck.py), and the two callers use it around their native calls"""
    rc, out = check_progress_glue(tmp_path)
    assert rc == 0 and "0 finding(s)" in out, out
    for rel, call in (("match/GpuFastqKMerMatcher.java", "GsGpuNative.hostMatchRun("), ("bloom/GpuFastqBloomFilter.java", "GsGpuNative.hostFilterFiles(")):
        src = open(os.path.join(ROOT, "java", "src", "org", "metagene", "genestrip", rel)).read()
        at = src.index(call)
        assert "isRequiresProgress()" in src[:at] and "new GpuProgress(" in src[:at] and "GpuProgress.translate(e)" in src[at:] and "progress.close()" in src[at:], rel
