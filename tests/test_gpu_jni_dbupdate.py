"""The dbUpdate* natives of java/jni/gsgpu_jni.c below the JVM, through the functional stand-in JNIEnv (tests/native/jni_stub) as
tests/test_gpu_jni_dbquality.py drives the dbQuality* ones: begin -> add -> finish -> fetch equals the ctypes path and the CPU
restatement; a direct buffer shorter than its element count raises before the library is called."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import genestrip_amd as ga
import qualitycheck as qc
from genestrip_amd import host, synth
from conftest import ROOT
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

PFX = "Java_org_metagene_genestrip_gpu_GsGpuNative_"


@pytest.fixture(scope="module")
def jni(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jniu") / "libgsjni_update_test.so")
    ga.lib()
    host.lib()
    cmd = ["gcc", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(ROOT, "tests", "native", "jni_stub"), "-I" + os.path.join(ROOT, "include"), "-o", out,
           os.path.join(ROOT, "java", "jni", "gsgpu_jni.c"), os.path.join(ROOT, "tests", "native", "jni_stub", "jni_env.c"),
           "-L" + os.path.join(ROOT, "genestrip_amd"), "-lgshost", "-lgsgpu", "-Wl,-rpath," + os.path.join(ROOT, "genestrip_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(out)
    vp, i64, i32, u8 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint8
    L.stub_env.restype = vp
    L.stub_buffer.restype, L.stub_buffer.argtypes = vp, [vp, i64]
    L.stub_take_exception.restype = C.c_char_p
    for name, res, args in (("dbUpdateBegin0", i64, [vp, vp, i32, i32, i32, vp, i64, u8, i32, i32, vp, i64, vp, i64, i64]),
                            ("dbUpdateBeginDb", i64, [vp, vp, i64, u8, i32, i32]),
                            ("dbUpdateAdd0", None, [vp, vp, i64, vp, i64, vp, i64, vp, i64, i64]),
                            ("dbUpdateFinish", i64, [vp, vp, i64]), ("dbUpdateSize", i64, [vp, vp, i64]),
                            ("dbUpdateFetch0", None, [vp, vp, i64, vp, i64, vp, i64]), ("dbUpdateToDb", i64, [vp, vp, i64]),
                            ("dbUpdateDestroy", None, [vp, vp, i64])):
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, args
    return L


def _buf(L, a):
    return L.stub_buffer(a.ctypes.data_as(C.c_void_p), a.nbytes)


def test_update_natives_through_the_jni_shim(jni):
    L, env = jni, jni.stub_env()
    sdb = synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)
    g = sdb.genomes
    nv = sdb.n_values
    parent = np.ascontiguousarray(sdb.parent_vi, dtype=np.int32)
    regions = [(g[i].tobytes(), int(sdb.species_vi[i])) for i in range(g.shape[0])]
    seq, off = qc.pack([s for s, _ in regions])
    seq = seq.copy()
    nodes = np.array([n for _, n in regions], np.int32)
    n = len(nodes)
    # the CPU restatement in stages: the store after the fill, then after the update
    ob = orc.DbBuild(31, nv, parent)
    ob.fill(seq, off, nodes)
    ob.optimize()
    wk, before = ob.fetch()
    ob.update(seq, off, nodes)
    _, after = ob.fetch()
    ob.close()
    assert (after != before).sum() > 100
    # the Python binding's result
    pu = ga.DeviceDbUpdater.from_arrays(31, wk, before, nv, parent)
    pu.add(seq, off, nodes)
    p_moved = pu.finish()
    pk, pv = pu.fetch()
    pu.close()
    assert np.array_equal(pk, wk) and np.array_equal(pv, after)
    begin, add = getattr(L, PFX + "dbUpdateBegin0"), getattr(L, PFX + "dbUpdateAdd0")
    fetch = getattr(L, PFX + "dbUpdateFetch0")
    nk = len(wk)
    # short buffers at begin: refused before the library sees them
    for caps, needle in (((parent.nbytes - 4, wk.nbytes, before.nbytes), b"parentVi"), ((parent.nbytes, wk.nbytes - 8, before.nbytes), b"kmers"),
                         ((parent.nbytes, wk.nbytes, before.nbytes - 4), b"valueIdx")):
        h = begin(env, None, 0, 31, nv, _buf(L, parent), caps[0], 1, -1, 1, _buf(L, wk), caps[1], _buf(L, before), caps[2], nk)
        msg = L.stub_take_exception()
        assert not h and msg is not None and needle in msg, msg
    u = begin(env, None, 0, 31, nv, _buf(L, parent), parent.nbytes, 1, -1, 1, _buf(L, wk), wk.nbytes, _buf(L, before), before.nbytes, nk)
    assert L.stub_take_exception() is None and u
    assert getattr(L, PFX + "dbUpdateSize")(env, None, u) == nk
    for caps, needle in (((seq.nbytes - 1, off.nbytes, nodes.nbytes), b"bases"), ((seq.nbytes, off.nbytes - 8, nodes.nbytes), b"offsets"),
                         ((seq.nbytes, off.nbytes, nodes.nbytes - 4), b"nodeVi")):
        add(env, None, u, _buf(L, seq), caps[0], _buf(L, off), caps[1], _buf(L, nodes), caps[2], n)
        msg = L.stub_take_exception()
        assert msg is not None and needle in msg, msg
    add(env, None, u, None, 0, _buf(L, off), off.nbytes, _buf(L, nodes), nodes.nbytes, n)
    assert b"bases" in L.stub_take_exception()
    gk, gv = np.zeros(nk, np.int64), np.zeros(nk, np.int32)
    fetch(env, None, u, _buf(L, gk), gk.nbytes, _buf(L, gv), gv.nbytes)
    msg = L.stub_take_exception()
    assert msg is not None and b"gs_dbupdate_finish first" in msg  # a library error surfaces as the exception's message
    half = n // 2  # two batches
    add(env, None, u, _buf(L, seq), seq.nbytes, _buf(L, off[:half + 1].copy()), 8 * (half + 1), _buf(L, nodes[:half].copy()), 4 * half, half)
    assert L.stub_take_exception() is None
    off2 = (off[half:] - off[half]).astype(np.uint64)
    seq2 = seq[int(off[half]):].copy()
    nodes2 = nodes[half:].copy()
    add(env, None, u, _buf(L, seq2), seq2.nbytes, _buf(L, off2), off2.nbytes, _buf(L, nodes2), nodes2.nbytes, n - half)
    assert L.stub_take_exception() is None
    moved = getattr(L, PFX + "dbUpdateFinish")(env, None, u)
    assert L.stub_take_exception() is None and moved == p_moved == int((after != before).sum())
    fetch(env, None, u, _buf(L, gk), gk.nbytes - 8, _buf(L, gv), gv.nbytes)
    assert b"kmers" in L.stub_take_exception()
    fetch(env, None, u, _buf(L, gk), gk.nbytes, _buf(L, gv), gv.nbytes - 4)
    assert b"valueIdx" in L.stub_take_exception() and not gk.any()
    fetch(env, None, u, _buf(L, gk), gk.nbytes, _buf(L, gv), gv.nbytes)
    assert L.stub_take_exception() is None
    assert np.array_equal(gk, pk) and np.array_equal(gv, pv)
    # ... to a store on the device, and from that store again: nothing left to move
    db = getattr(L, PFX + "dbUpdateToDb")(env, None, u)
    assert L.stub_take_exception() is None and db
    getattr(L, PFX + "dbUpdateDestroy")(env, None, u)
    store = ga.DeviceKMerStore._wrap(C.c_void_p(db), 31, nv, 0)
    u2 = getattr(L, PFX + "dbUpdateBeginDb")(env, None, db, 1, -1, 1)
    assert L.stub_take_exception() is None and u2
    add(env, None, u2, _buf(L, seq), seq.nbytes, _buf(L, off), off.nbytes, _buf(L, nodes), nodes.nbytes, n)
    assert getattr(L, PFX + "dbUpdateFinish")(env, None, u2) == 0 and L.stub_take_exception() is None
    gk[:], gv[:] = 0, 0
    fetch(env, None, u2, _buf(L, gk), gk.nbytes, _buf(L, gv), gv.nbytes)
    assert L.stub_take_exception() is None and np.array_equal(gk, wk) and np.array_equal(gv, after)
    getattr(L, PFX + "dbUpdateDestroy")(env, None, u2)
    store.close()
