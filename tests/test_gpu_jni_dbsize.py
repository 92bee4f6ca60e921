"""The dbSize* natives of java/jni/gsgpu_jni.c below the JVM, through the functional stand-in JNIEnv (tests/native/jni_stub) as
tests/test_gpu_jni_dbquality.py drives the dbQuality* ones: direct ByteBuffers in, counts out, equal to the ctypes path and the CPU
reference on one small case; a buffer one byte shorter than what the call needs raises instead of being read or written out of
bounds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import genestrip_amd as ga
import sizecheck as sc
from genestrip_amd import host
from conftest import ROOT

pytestmark = pytest.mark.gpu

PFX = "Java_org_metagene_genestrip_gpu_GsGpuNative_"
K, NV, HB, RB = 21, 3, 6, 16


@pytest.fixture(scope="module")
def jni(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jnis") / "libgsjni_size_test.so")
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
    for name, res, args in (("dbSizeBegin", i64, [vp, vp, i32, i32, i32, u8, i32, i32, i32, i32, u8]), ("dbSizeSetRange", None, [vp, vp, i64, i64, i64]),
                            ("dbSizeAdd0", None, [vp, vp, i64, vp, i64, vp, i64, vp, i64, i64]),
                            ("dbSizeCounts0", None, [vp, vp, i64, vp, i64, vp, i64, vp, i64]), ("dbSizeDistinct0", i64, [vp, vp, i64, vp, i64]),
                            ("dbSizePlan0", i32, [vp, vp, vp, i64, i32, i32, i64, vp, i64, i32]), ("dbSizeDestroy", None, [vp, vp, i64])):
        f = getattr(L, PFX + name)
        f.restype, f.argtypes = res, args
    return L


def _buf(L, a):
    return L.stub_buffer(a.ctypes.data_as(C.c_void_p), a.nbytes)


def test_size_natives_through_the_jni_shim(jni):
    L, env = jni, jni.stub_env()
    rng = np.random.default_rng(21)
    g = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 1500))
    regions = [(g, 0), (g[200:900], 1), (g[::-1], 2), (b"AC" * 30 + g[:100], 1)]
    ref = sc.count(K, regions, NV, True, 1, 20, HB)
    n_ref, buckets_ref = sc.distinct(ref.keys, RB)
    seq, off = sc.pack([s for s, _ in regions])
    seq = seq.copy()
    tags = np.array([t for _, t in regions], np.int32)
    n = len(tags)
    s = getattr(L, PFX + "dbSizeBegin")(env, None, 0, K, NV, 1, 20, 1, HB, RB, 1)
    assert L.stub_take_exception() is None and s
    add, counts, distinct, plan = (getattr(L, PFX + x) for x in ("dbSizeAdd0", "dbSizeCounts0", "dbSizeDistinct0", "dbSizePlan0"))
    # short buffers: refused before the library sees them
    for caps, needle in (((seq.nbytes - 1, off.nbytes, tags.nbytes), b"bases"), ((seq.nbytes, off.nbytes - 1, tags.nbytes), b"offsets"),
                         ((seq.nbytes, off.nbytes, tags.nbytes - 1), b"tagVi")):
        add(env, None, s, _buf(L, seq), caps[0], _buf(L, off), caps[1], _buf(L, tags), caps[2], n)
        msg = L.stub_take_exception()
        assert msg is not None and needle in msg, msg
    add(env, None, s, None, 0, _buf(L, off), off.nbytes, _buf(L, tags), tags.nbytes, n)
    assert b"bases" in L.stub_take_exception()
    add(env, None, s, _buf(L, seq), seq.nbytes, _buf(L, off), off.nbytes, _buf(L, tags), tags.nbytes, n)
    assert L.stub_take_exception() is None
    totals, per_value, hist = np.zeros(3, np.int64), np.zeros(NV, np.int64), np.zeros(1 << HB, np.int64)
    for caps, needle in (((totals.nbytes - 1, per_value.nbytes, hist.nbytes), b"totals"), ((totals.nbytes, per_value.nbytes - 1, hist.nbytes), b"perValue"),
                         ((totals.nbytes, per_value.nbytes, hist.nbytes - 1), b"hist")):
        counts(env, None, s, _buf(L, totals), caps[0], _buf(L, per_value), caps[1], _buf(L, hist), caps[2])
        msg = L.stub_take_exception()
        assert msg is not None and needle in msg, msg
    assert not totals.any() and not per_value.any() and not hist.any()
    counts(env, None, s, _buf(L, totals), totals.nbytes, _buf(L, per_value), per_value.nbytes, _buf(L, hist), hist.nbytes)
    assert L.stub_take_exception() is None
    assert totals.tolist() == [ref.total, ref.dust, ref.included] and ref.dust > 0
    assert np.array_equal(per_value, ref.per_value) and np.array_equal(hist, ref.hist)
    buckets = np.zeros(1 << RB, np.int64)
    assert distinct(env, None, s, _buf(L, buckets), buckets.nbytes - 1) == 0 and b"bucketSizes" in L.stub_take_exception()
    assert distinct(env, None, s, None, 0) == 0 and b"bucketSizes" in L.stub_take_exception()
    assert not buckets.any()
    assert distinct(env, None, s, _buf(L, buckets), buckets.nbytes) == n_ref and L.stub_take_exception() is None
    assert np.array_equal(buckets, buckets_ref)
    # the ctypes path on the same case
    d = ga.DeviceDbSizer(K, NV, max_dust=20, hist_bits=HB, radix_bits=RB, keep_keys=True)
    d.add(seq, off, tags)
    t, pv, h = d.counts()
    assert [t.total, t.dust, t.included] == totals.tolist() and np.array_equal(pv, per_value) and np.array_equal(h, hist)
    n_d, b_d = d.distinct()
    assert n_d == n_ref and np.array_equal(b_d, buckets)
    d.close()
    # a library error surfaces as the exception's message: add after distinct
    add(env, None, s, _buf(L, seq), seq.nbytes, _buf(L, off), off.nbytes, _buf(L, tags), tags.nbytes, n)
    msg = L.stub_take_exception()
    assert msg is not None and b"gs_dbsize_set_range" in msg
    # the plan, and the next pass on the same handle over its first range
    max_pairs = ref.included // 2 + int(ref.hist.max())
    want = ga.plan_ranges(hist, HB, K, max_pairs)
    bounds = np.zeros(len(hist) + 1, np.uint64)
    assert plan(env, None, _buf(L, hist), hist.nbytes - 1, HB, K, max_pairs, _buf(L, bounds), bounds.nbytes, len(hist)) == 0
    assert b"hist" in L.stub_take_exception()
    assert plan(env, None, _buf(L, hist), hist.nbytes, HB, K, max_pairs, _buf(L, bounds), bounds.nbytes - 1, len(hist)) == 0
    assert b"bounds" in L.stub_take_exception() and not bounds.any()
    nr = plan(env, None, _buf(L, hist), hist.nbytes, HB, K, max_pairs, _buf(L, bounds), bounds.nbytes, len(hist))
    assert L.stub_take_exception() is None and nr == len(want) >= 2
    assert [(int(bounds[i]), int(bounds[i + 1])) for i in range(nr)] == want
    assert plan(env, None, _buf(L, hist), hist.nbytes, HB, K, 1, _buf(L, bounds), bounds.nbytes, len(hist)) == 0
    assert b"bin " in L.stub_take_exception()
    lo, hi = want[0]
    getattr(L, PFX + "dbSizeSetRange")(env, None, s, lo, hi)
    assert L.stub_take_exception() is None
    add(env, None, s, _buf(L, seq), seq.nbytes, _buf(L, off), off.nbytes, _buf(L, tags), tags.nbytes, n)
    assert distinct(env, None, s, _buf(L, buckets), buckets.nbytes) == sc.distinct([x for x in ref.keys if lo <= x < hi])[0]
    assert L.stub_take_exception() is None
    getattr(L, PFX + "dbSizeDestroy")(env, None, s)
