"""The sizing pass without a GPU: the plan is host arithmetic (gs_dbsize_plan), the CPU reference of the GPU tests
(tests/sizecheck.py) is pinned against the oracle, and the compute entry points refuse to run without a device."""
import ctypes as C

import numpy as np
import pytest

import genestrip_amd as ga
import sizecheck as sc
from oracle import gs_oracle as orc

INVALID, NODEVICE = -1, -6


def _plan(hist, hist_bits, k, max_pairs, cap=None):
    """-> (rc, bounds as Python ints, message)"""
    h = np.ascontiguousarray(hist, dtype=np.int64)
    cap = len(h) if cap is None else cap
    bounds = np.zeros(cap + 1, dtype=np.uint64)
    n = C.c_int(-1)
    rc = ga.lib().gs_dbsize_plan(h.ctypes.data_as(C.c_void_p), hist_bits, k, max_pairs, bounds.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return rc, [int(b) for b in bounds[:n.value + 1]], (ga.lib().gs_last_error() or b"").decode()


def _sums(hist, bounds, shift):
    return [int(np.sum(hist[(lo >> shift):(hi >> shift)])) for lo, hi in zip(bounds[:-1], bounds[1:])]


def test_dust_window_form_equals_the_oracle():
    """the golden k-mers of DESIGN section 4a, then a few hundred random ones with runs and short periods"""
    assert [sc.fib(i) for i in range(7)] == [0, 1, 2, 3, 5, 8, 13]
    assert sc.dust_window("TTTCGCGA") == orc.dust_value("TTTCGCGA") == sc.fib(2) + sc.fib(1) + sc.fib(2)
    assert sc.dust_window("AC" * 15 + "A") == orc.dust_value("AC" * 15 + "A") == sc.fib(29)
    assert sc.dust_window("C" * 31) == orc.dust_value("C" * 31) == sc.fib(30) + sc.fib(29) + sc.fib(28)
    rng = np.random.default_rng(5)
    for _ in range(300):
        k = int(rng.integers(1, 32))
        unit = "".join(rng.choice(list("ACGT"), int(rng.integers(1, 4))))
        w = list((unit * 31)[:k])
        for i in rng.integers(0, k, int(rng.integers(0, 4))):
            w[i] = "ACGT"[int(rng.integers(4))]
        w = "".join(w)
        assert sc.dust_window(w) == orc.dust_value(w), w


def test_sizecheck_distinct_equals_the_oracle_build():
    rng = np.random.default_rng(6)
    g = bytes(rng.choice(list(b"ACGT"), 400).astype(np.uint8))
    regions = [(g, 0), (g[50:300] + b"N" + g[:40].lower(), 1), (b"AC" * 40, 0)]
    for k, step, max_dust, lower in ((5, 1, -1, True), (15, 2, 20, True), (31, 3, sc.fib(29) - 1, False)):
        ref = sc.count(k, regions, 2, lower, step, max_dust)
        assert ref.total == ref.dust + ref.included == ref.dust + int(ref.per_value.sum()) and ref.included == int(ref.hist.sum())
        assert np.array_equal(np.unique(np.array(ref.keys, np.int64)), sc.distinct_by_build(k, regions, lower, step, max_dust))


def test_plan_uniform_histogram():
    hist = np.full(64, 10, np.int64)
    rc, bounds, _ = _plan(hist, 6, 15, 40)
    assert rc == 0 and bounds == [i << 24 for i in range(0, 64, 4)] + [1 << 30]
    assert ga.plan_ranges(hist, 6, 15, 40) == list(zip(bounds[:-1], bounds[1:]))
    rc, bounds, _ = _plan(hist, 6, 15, 640)
    assert rc == 0 and bounds == [0, 1 << 30]


def test_plan_a_bin_at_and_above_max_pairs():
    hist = np.array([3, 100, 0, 7], np.int64)
    rc, bounds, _ = _plan(hist, 2, 10, 100)
    assert rc == 0 and bounds == [0, 1 << 18, 3 << 18, 1 << 20]  # [3] [100, 0] [7]: the full bin fits, the empty one joins it
    hist[1] = 101
    rc, bounds, msg = _plan(hist, 2, 10, 100)
    assert rc == INVALID and bounds == [0]
    assert "bin 1 " in msg and "101" in msg and "100" in msg, msg
    with pytest.raises(ga.GsError) as e:
        ga.plan_ranges(hist, 2, 10, 100)
    assert e.value.code == INVALID and "bin 1 " in str(e.value)


def test_plan_zeros_and_empty_bins_at_the_ends():
    rc, bounds, _ = _plan(np.zeros(256, np.int64), 8, 21, 1)
    assert rc == 0 and bounds == [0, 1 << 42]
    hist = np.zeros(16, np.int64)
    hist[5], hist[6], hist[9] = 4, 4, 4
    rc, bounds, _ = _plan(hist, 4, 4, 4)
    assert rc == 0 and bounds == [0, 6 << 4, 9 << 4, 1 << 8]  # leading empties join the first range, trailing ones the last
    assert _sums(hist, bounds, 4) == [4, 4, 4]


def test_plan_more_hist_bits_than_key_bits():
    """hist_bits = 12 with k = 3: hb = 6, one bin per k-mer"""
    hist = np.arange(64, dtype=np.int64) % 3
    rc, bounds, _ = _plan(hist, 12, 3, 2)
    assert rc == 0 and bounds[0] == 0 and bounds[-1] == 64 and all(s <= 2 for s in _sums(hist, bounds, 0))
    assert len(bounds) - 1 == sc.greedy_ranges(hist, 2)
    with pytest.raises(ValueError):
        ga.plan_ranges(np.zeros(4096, np.int64), 12, 3, 2)  # (the histogram of this k has 64 bins)


def test_plan_cap_one_too_small():
    hist = np.full(8, 5, np.int64)
    rc, bounds, _ = _plan(hist, 3, 9, 10, cap=4)
    assert rc == 0 and len(bounds) == 5
    rc, bounds, msg = _plan(hist, 3, 9, 10, cap=3)
    assert rc == INVALID and "cap" in msg, msg


def test_plan_invariants_on_random_histograms():
    rng = np.random.default_rng(11)
    for i in range(200):
        hb = int(rng.integers(1, 13))
        k = int(rng.integers((hb + 1) // 2, 32))
        hist = rng.integers(0, 1000, 1 << hb) * (rng.random(1 << hb) < rng.random())
        max_pairs = int(max(hist.max(), 1) + rng.integers(0, 3000))
        rc, bounds, msg = _plan(hist, hb, k, max_pairs)
        assert rc == 0, msg
        shift = 2 * k - hb
        assert bounds[0] == 0 and bounds[-1] == 1 << (2 * k) and all(a < b for a, b in zip(bounds[:-1], bounds[1:]))
        assert all(b % (1 << shift) == 0 for b in bounds)
        sums = _sums(hist, bounds, shift)
        assert sum(sums) == int(hist.sum()) and all(s <= max_pairs for s in sums)
        assert len(bounds) - 1 == sc.greedy_ranges(hist, max_pairs)


def test_plan_refuses_bad_arguments():
    hist = np.ones(4, np.int64)
    assert _plan(hist, 0, 5, 1)[0] == INVALID and _plan(hist, 13, 5, 1)[0] == INVALID
    assert _plan(hist, 2, 0, 1)[0] == INVALID and _plan(hist, 2, 32, 1)[0] == INVALID
    assert _plan(hist, 2, 5, 0)[0] == INVALID and _plan(hist, 2, 5, 1, cap=0)[0] == INVALID
    assert _plan(np.array([1, -1, 0, 0], np.int64), 2, 5, 1)[0] == INVALID


def test_exports():
    assert ga.DeviceDbSizer.__name__ == "DeviceDbSizer" and callable(ga.plan_ranges)
    assert "DeviceDbSizer" in ga.__all__ and "plan_ranges" in ga.__all__
    for name in ("begin", "set_range", "add", "counts", "distinct", "get_stats", "destroy", "plan"):
        assert "gs_dbsize_" + name in ga.ABI_SYMBOLS


def test_binding_argument_checks_need_no_device():
    with pytest.raises(ValueError):
        ga.DeviceDbSizer(21, hist_bits=0)
    with pytest.raises(ValueError):
        ga.DeviceDbSizer(21, hist_bits=13)
    with pytest.raises(ValueError):
        ga.DeviceDbSizer(21, radix_bits=15, keep_keys=True)
    with pytest.raises(ValueError):
        ga.DeviceDbSizer(21, radix_bits=25, keep_keys=True)
    with pytest.raises(ValueError):
        ga.plan_ranges(np.zeros(3, np.int64), 2, 5, 1)
    with pytest.raises(ValueError):
        ga.plan_ranges(np.zeros(4, np.int64), 2, 32, 1)


def test_begin_checks_its_arguments_before_it_looks_for_a_device():
    L = ga.lib()
    h = C.c_void_p(1)
    for args, msg in (((0, 1, 1, -1, 1, 12, 0, 0), "k must be in [1,31]"), ((21, 0, 1, -1, 1, 12, 0, 0), "n_values must be in [1, 2^24]"),
                      ((21, 1, 1, -1, 0, 12, 0, 0), "stepSize must be >= 1 (C/GSConfigKey.java:236)"),
                      ((21, 1, 1, -1, 1, 13, 0, 0), "hist_bits must be in [1,12]"),
                      ((21, 1, 1, -1, 1, 12, 15, 1), "radix_bits must be 0 or in [16,24] (GSConfigKey.RADIX_STORE_BITS)")):
        h.value = 1
        assert L.gs_dbsize_begin(C.byref(h), 0, *args) == INVALID
        assert (L.gs_last_error() or b"").decode() == msg and not h.value
    assert L.gs_dbsize_begin(None, 0, 21, 1, 1, -1, 1, 12, 0, 0) == INVALID


def test_begin_without_a_gpu_is_the_no_device_code():
    """(with a device the same call opens a handle: tests/test_gpu_dbsize.py goes on from there)"""
    L = ga.lib()
    h = C.c_void_p(1)
    rc = L.gs_dbsize_begin(C.byref(h), 0, 21, 1, 1, -1, 1, 12, 16, 1)
    if ga.device_count() > 0:
        assert rc == 0 and h.value and L.gs_dbsize_destroy(h) == 0
        return
    assert rc == NODEVICE and not h.value
    with pytest.raises(ga.GsError) as e:
        ga.DeviceDbSizer(21)
    assert e.value.code == NODEVICE
