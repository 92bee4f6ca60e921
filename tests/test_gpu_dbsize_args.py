"""The project's table of defective region batches (tests/test_gpu_region_args.py) applied to the fourth family that takes
regions, gs_dbsize_add: each defect is refused with its code and the exact gs_last_error() text, the counters are as they were,
and the handle then gives the result of a handle that never saw the defect.  Needs an MI355X: run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import genestrip_amd as ga
import sizecheck as sc

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
K, NV = 21, 4

BAD_ARGUMENT = "bad argument"
BAD_MEM = "mem must be GS_MEM_HOST or GS_MEM_DEVICE"
OFF_FIRST = "offsets[0] must be 0"
OFF_ORDER = "offsets must not decrease"
NOT_A_VALUE = "tag_vi: not a value index"


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _last_error():
    return (ga.lib().gs_last_error() or b"").decode()


class Case:
    def __init__(self):
        rng = np.random.default_rng(4242)
        parts = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in (150, 90, 200, 64, 33)]
        self.tags = np.array([0, 1, 2, 3, 1], np.int32)
        self.seq, self.off = sc.pack(parts)
        self.n = len(parts)
        self.ref = sc.count(K, list(zip(parts, self.tags)), NV, hist_bits=6)


@pytest.fixture(scope="module")
def case():
    return Case()


def _open():
    return ga.DeviceDbSizer(K, NV, hist_bits=6, radix_bits=16, keep_keys=True)


def _add(h, seq, off, tags, n, mem):
    return ga.lib().gs_dbsize_add(h.h, _p(seq), _p(off), _p(tags), n, mem)


def _state(h):
    t, per_value, hist = h.counts()
    return (t.total, t.dust, t.included, per_value.tolist(), hist.tolist(), h.stats().n_keys)


def _clean(c):
    return (c.ref.total, c.ref.dust, c.ref.included, c.ref.per_value.tolist(), c.ref.hist.tolist(), c.ref.included)


def _with(c, **change):
    a = dict(seq=c.seq, off=c.off, tags=c.tags, n=c.n, mem=ga.MEM_HOST)
    a.update(change)
    return a["seq"], a["off"], a["tags"], a["n"], a["mem"]


def _tag(c, v):
    t = c.tags.copy()
    t[1] = v
    return t


def _off_first(c):
    return c.off + np.uint64(1)


def _off_decreasing(c):
    o = c.off.copy()
    o[2] = o[1] - np.uint64(1)
    return o


DEFECTS = [
    ("bad mem", lambda c: _with(c, mem=7), BAD_MEM),
    ("offsets[0] != 0", lambda c: _with(c, off=_off_first(c)), OFF_FIRST),
    ("decreasing offsets", lambda c: _with(c, off=_off_decreasing(c)), OFF_ORDER),
    ("a tag of n_values", lambda c: _with(c, tags=_tag(c, NV)), NOT_A_VALUE),
    ("a tag of -1", lambda c: _with(c, tags=_tag(c, -1)), NOT_A_VALUE),
    ("NULL seq", lambda c: _with(c, seq=None), BAD_ARGUMENT),
    ("NULL offsets", lambda c: _with(c, off=None), BAD_ARGUMENT),
    ("NULL tags", lambda c: _with(c, tags=None), BAD_ARGUMENT),
    ("negative n_regions", lambda c: _with(c, n=-1), BAD_ARGUMENT),
    # several defects in one call: mem, then tags, then offsets
    ("bad mem and a bad tag", lambda c: _with(c, mem=7, tags=_tag(c, NV)), BAD_MEM),
    ("bad mem and bad offsets", lambda c: _with(c, mem=-1, off=_off_first(c)), BAD_MEM),
    ("a bad tag and bad offsets", lambda c: _with(c, tags=_tag(c, NV), off=_off_decreasing(c)), NOT_A_VALUE),
]


@pytest.mark.parametrize("name,batch,message", DEFECTS, ids=[d[0] for d in DEFECTS])
@pytest.mark.parametrize("after_an_add", [False, True])
def test_a_defective_batch_is_refused_and_counts_are_unchanged(case, name, batch, message, after_an_add):
    h = _open()
    if after_an_add:
        assert _add(h, *_with(case)) == OK, _last_error()
    before = _state(h)
    assert before == (_clean(case) if after_an_add else (0, 0, 0, [0] * NV, [0] * 64, 0))
    assert (_add(h, *batch(case)), _last_error()) == (INVALID, message)
    assert _state(h) == before
    if not after_an_add:
        assert _add(h, *_with(case)) == OK, _last_error()
    assert _state(h) == _clean(case)
    assert h.distinct()[0] == sc.distinct(case.ref.keys)[0]
    h.close()


@pytest.mark.parametrize("pointers", [True, False])
def test_no_regions_is_ok_and_changes_nothing(case, pointers):
    h = _open()
    args = _with(case, n=0) if pointers else (None, None, None, 0, ga.MEM_HOST)
    assert _add(h, *args) == OK
    assert _add(h, *args[:4], 7) == OK  # (nothing is looked at: not even mem)
    assert _state(h) == (0, 0, 0, [0] * NV, [0] * 64, 0)
    assert ga.lib().gs_dbsize_set_range(h.h, 0, 2 ** 64 - 1) == OK  # (still before the first add)
    assert _add(h, *_with(case)) == OK, _last_error()
    assert _state(h) == _clean(case)
    h.close()
    h = _open()
    assert _add(h, *args) == OK
    n, buckets = h.distinct()
    assert n == 0 and not buckets.any()
    h.close()


def test_null_handles_and_outputs():
    L = ga.lib()
    assert (L.gs_dbsize_add(None, None, None, None, 0, 0), _last_error()) == (INVALID, BAD_ARGUMENT)
    assert L.gs_dbsize_counts(None, None, None, None) == INVALID and L.gs_dbsize_distinct(None, None, None) == INVALID
    assert L.gs_dbsize_set_range(None, 0, 1) == INVALID and L.gs_dbsize_get_stats(None, None) == INVALID
    assert L.gs_dbsize_destroy(None) == OK
    h = _open()
    assert L.gs_dbsize_set_range(h.h, 5, 5) == INVALID and L.gs_dbsize_counts(h.h, None, None, None) == INVALID
    n = C.c_int64(0)
    assert L.gs_dbsize_distinct(h.h, C.byref(n), None) == INVALID  # (radix_bits 16 needs the bucket array)
    t = ga.binding.DbSizeTotals()
    assert L.gs_dbsize_counts(h.h, C.byref(t), None, None) == OK  # per_value and hist are optional
    h.close()
