"""The dbQuality* natives of java/jni/gsgpu_jni.c below the JVM, through the functional stand-in JNIEnv (tests/native/jni_stub) as
tests/test_gpu_jni.py drives the others: direct ByteBuffers in, counts out, equal to the ctypes path and the CPU reference; a buffer
shorter than what the call needs raises instead of being read or written out of bounds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import genestrip_amd as ga
import qualitycheck as qc
from genestrip_amd import host, synth
from conftest import ROOT

pytestmark = pytest.mark.gpu

PFX = "Java_org_metagene_genestrip_gpu_GsGpuNative_"


@pytest.fixture(scope="module")
def jni(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jniq") / "libgsjni_quality_test.so")
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
    for name, res, args in (("dbQualityBegin", i64, [vp, vp, i64, u8, i32, i32]), ("dbQualitySetRange", None, [vp, vp, i64, i64, i64]),
                            ("dbQualityAdd0", None, [vp, vp, i64, vp, i64, vp, i64, vp, i64, i64]),
                            ("dbQualityFinish0", None, [vp, vp, i64, i32, vp, i64, vp, i64]), ("dbQualityDestroy", None, [vp, vp, i64])):
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, args
    return L


def _buf(L, a):
    return L.stub_buffer(a.ctypes.data_as(C.c_void_p), a.nbytes)


def test_quality_natives_through_the_jni_shim(jni):
    L, env = jni, jni.stub_env()
    sdb = synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)
    g = sdb.genomes
    nv = sdb.n_values
    store = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, nv, sdb.parent_vi)
    regions = [(g[i].tobytes(), int(sdb.species_vi[i])) for i in range(g.shape[0])]
    ref = qc.reference_counts(31, sdb.kmers, sdb.value_idx, sdb.parent_vi, regions)
    seq, off = qc.pack([s for s, _ in regions])
    seq = seq.copy()
    leaf = np.array([l for _, l in regions], np.int32)
    n = len(leaf)
    q = getattr(L, PFX + "dbQualityBegin")(env, None, store.h.value, 1, -1, 1)
    assert L.stub_take_exception() is None and q
    add, fin = getattr(L, PFX + "dbQualityAdd0"), getattr(L, PFX + "dbQualityFinish0")
    # short buffers: refused before the library sees them
    for caps, needle in (((seq.nbytes - 1, off.nbytes, leaf.nbytes), b"bases"), ((seq.nbytes, off.nbytes - 8, leaf.nbytes), b"offsets"),
                         ((seq.nbytes, off.nbytes, leaf.nbytes - 4), b"leafVi")):
        add(env, None, q, _buf(L, seq), caps[0], _buf(L, off), caps[1], _buf(L, leaf), caps[2], n)
        msg = L.stub_take_exception()
        assert msg is not None and needle in msg, msg
    add(env, None, q, None, 0, _buf(L, off), off.nbytes, _buf(L, leaf), leaf.nbytes, n)
    assert b"bases" in L.stub_take_exception()
    add(env, None, q, _buf(L, seq), seq.nbytes, _buf(L, off), off.nbytes, _buf(L, leaf), leaf.nbytes, n)
    assert L.stub_take_exception() is None
    counts, present = np.zeros((nv, 3), np.int64), np.zeros(nv, np.uint8)
    fin(env, None, q, nv, _buf(L, counts), counts.nbytes - 8, _buf(L, present), present.nbytes)
    assert b"counts" in L.stub_take_exception()
    fin(env, None, q, nv, _buf(L, counts), counts.nbytes, _buf(L, present), present.nbytes - 1)
    assert b"present" in L.stub_take_exception() and not counts.any()
    fin(env, None, q, nv, _buf(L, counts), counts.nbytes, _buf(L, present), present.nbytes)
    assert L.stub_take_exception() is None
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(present, ref["present"]) and present.sum() == 9
    # a library error surfaces as the exception's message: add after finish
    add(env, None, q, _buf(L, seq), seq.nbytes, _buf(L, off), off.nbytes, _buf(L, leaf), leaf.nbytes, n)
    msg = L.stub_take_exception()
    assert msg is not None and b"gs_dbquality_finish" in msg
    # the next pass on the same handle, over the upper half of the k-mers
    lo, hi = ga.binding.kmer_ranges(31, 2)[1]
    getattr(L, PFX + "dbQualitySetRange")(env, None, q, lo, hi)
    assert L.stub_take_exception() is None
    add(env, None, q, _buf(L, seq), seq.nbytes, _buf(L, off), off.nbytes, _buf(L, leaf), leaf.nbytes, n)
    fin(env, None, q, nv, _buf(L, counts), counts.nbytes, _buf(L, present), present.nbytes)
    assert L.stub_take_exception() is None
    half = qc.reference_counts(31, sdb.kmers, sdb.value_idx, sdb.parent_vi, regions, lo=lo, hi=hi)
    assert np.array_equal(counts, half["counts"]) and np.array_equal(present, half["present"])
    getattr(L, PFX + "dbQualityDestroy")(env, None, q)
    store.close()
