"""gs_dbsize against tests/sizecheck.py, bit for bit: the counting kernel at the region, tile and tag boundaries, the noise
bytes, both sides of the DUST gate, every histogram width, batching and memory kinds, the distinct pass, and the plan it gives
to gs_dbbuild.  Every test runs under GS_SIZE_GRID=2 unless it says otherwise: two workgroups, so a few hundred bases wrap the
grid-stride loop and both workgroups flush.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import genestrip_amd as ga
import sizecheck as sc

pytestmark = pytest.mark.gpu

STATE = -5
NV = 5


@pytest.fixture(autouse=True)
def _grid(monkeypatch):
    monkeypatch.setenv("GS_SIZE_GRID", "2")


def _rand(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def _run(k, regions, n_values=NV, per_region=False, device=False, **kw):
    """regions: list of (bytes, tag) -> (totals, per_value, hist) of one pass"""
    s = ga.DeviceDbSizer(k, n_values, **kw)
    _add(s, regions, per_region, device)
    out = s.counts()
    s.close()
    return out


def _add(s, regions, per_region=False, device=False):
    for batch in ([[r] for r in regions] if per_region else [regions]):
        seq, off = sc.pack([r for r, _ in batch])
        tags = np.array([t for _, t in batch], np.int32)
        if device:
            import torch
            s.add(torch.from_numpy(seq.copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), tags)
        else:
            s.add(seq, off, tags)


def _equal(got, ref):
    t, per_value, hist = got
    assert (t.total, t.dust, t.included) == (ref.total, ref.dust, ref.included)
    assert np.array_equal(per_value, ref.per_value)
    assert np.array_equal(hist, ref.hist)
    assert int(hist.sum()) == t.included == int(per_value.sum())


def _boundary_regions(k, seed):
    """tiles that see a region start, a region end, several regions and no region; tags cycle, so tiles hold several tags"""
    rng = np.random.default_rng(seed)
    lengths = [0, 1, k - 1, k, k + 1, 63, 64, 65, 64 + k - 2, 64 + k - 1, 64 + k, 127 + k]
    return [(_rand(rng, max(n, 0)), i % NV) for i, n in enumerate(lengths)]


@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("k", [1, 2, 15, 16, 31])
def test_region_lengths_around_k_and_the_tile(k, step):
    regions = _boundary_regions(k, 100 + k)
    ref = sc.count(k, regions, NV, True, step)
    assert ref.included > 0
    _equal(_run(k, regions, step_size=step), ref)


@pytest.mark.parametrize("lower", [False, True])
def test_noise_bytes(lower):
    k = 15
    rng = np.random.default_rng(7)
    g = _rand(rng, 200)
    last = len(g) - 1
    regions = [(g[:90] + b"N" + g[90:], 0), (g.lower(), 1), (g[:70] + g[70:130].lower() + g[130:], 2), (g[:100] + b"\r" + g[100:], 3),
               (b"N" * 80, 4), (b"n" * 3, 4)]
    for at in (0, k - 1, 63, 64, last):  # a non-base at the offsets where a window, a tile or the region begins or ends
        regions.append((g[:at] + b"X" + g[at + 1:], at % NV))
    ref = sc.count(k, regions, NV, lower, 1)
    assert 0 < ref.included < sum(max(len(r) - k + 1, 0) for r, _ in regions)
    assert ref.per_value[1] == (len(g) - k + 1 if lower else 0)
    _equal(_run(k, regions, lower_case_bases=lower), ref)


@pytest.mark.parametrize("max_dust", [-1, 0, 20, sc.fib(29) - 1, sc.fib(29)])
def test_both_sides_of_the_dust_gate(max_dust):
    k = 31
    rng = np.random.default_rng(8)
    regions = [(b"C" * 70, 0), (b"AC" * 40, 1), (b"ACG" * 30, 2), (_rand(rng, 150), 3), (b"AC" * 20 + _rand(rng, 40) + b"T" * 35, 4),
               (b"ACGT" * 12, 0)]  # (period 4: a score of 0)
    ref = sc.count(k, regions, NV, True, 1, max_dust)
    if max_dust >= 0:
        assert ref.dust > 0 and ref.included > 0  # both sides occur
    else:
        assert ref.dust == 0
    # (AC)^15 A scores fib(29): dropped at fib(29) - 1, kept at fib(29)
    assert (ref.per_value[1] > 0) == (max_dust < 0 or max_dust >= sc.fib(29))
    _equal(_run(k, regions, max_dust=max_dust), ref)


@pytest.mark.parametrize("k,hist_bits", [(15, 1), (15, 6), (15, 12), (3, 12), (31, 12)])
def test_histogram_widths(k, hist_bits):
    rng = np.random.default_rng(9)
    regions = [(_rand(rng, 300), 0), (b"T" * 40 + _rand(rng, 100), 1)]
    ref = sc.count(k, regions, NV, True, 1, -1, hist_bits)
    assert len(ref.hist) == 1 << min(hist_bits, 2 * k) and np.count_nonzero(ref.hist) > 1
    _equal(_run(k, regions, hist_bits=hist_bits), ref)


def test_histogram_does_not_depend_on_the_grid(monkeypatch):
    """~6 kb under one workgroup, two, and the default grid"""
    k = 21
    rng = np.random.default_rng(10)
    regions = [(_rand(rng, 2500), 0), (_rand(rng, 37), 1), (_rand(rng, 3500), 2)]
    ref = sc.count(k, regions, NV, True, 1, -1, 12)
    for grid in ("1", "2", None):
        if grid is None:
            monkeypatch.delenv("GS_SIZE_GRID")
        else:
            monkeypatch.setenv("GS_SIZE_GRID", grid)
        _equal(_run(k, regions), ref)


def test_batching_memory_kind_and_a_second_pass():
    k = 16
    regions = _boundary_regions(k, 11)
    ref = sc.count(k, regions, NV, True, 2, 20)
    kw = dict(step_size=2, max_dust=20)
    _equal(_run(k, regions, **kw), ref)
    _equal(_run(k, regions, per_region=True, **kw), ref)
    _equal(_run(k, regions, device=True, **kw), ref)
    _equal(_run(k, regions, per_region=True, device=True, **kw), ref)
    # one handle, two passes: the second starts from zero; a range changes no count
    s = ga.DeviceDbSizer(k, NV, **kw)
    _add(s, regions)
    assert ga.lib().gs_dbsize_set_range(s.h, 0, 1 << 20) == STATE  # (adds, but no counts / distinct yet)
    _equal(s.counts(), ref)
    _add(s, regions[:3])  # counts() reads, the pass goes on
    s.counts()
    s.set_range(1 << 10, 1 << 20)
    t, per_value, hist = s.counts()
    assert (t.total, t.dust, t.included) == (0, 0, 0) and not per_value.any() and not hist.any()
    _add(s, regions, per_region=True)
    _equal(s.counts(), ref)
    st = s.stats()
    assert st.n_bases == sum(len(r) for r, _ in regions) and st.n_regions == len(regions) and st.n_keys == 0 and st.bytes_peak == 0
    s.close()


@pytest.fixture(scope="module")
def genomes():
    """two copies of a 3 kb genome, its reverse complement and a mutated copy: duplicates within and across regions and strands"""
    rng = np.random.default_rng(12)
    g = _rand(rng, 3000)
    rc = g[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
    m = bytearray(g)
    for at in rng.integers(0, len(g), 60):
        m[at] = b"ACGT"[int(rng.integers(4))]
    regions = [(g, 0), (g, 1), (rc, 2), (bytes(m), 3)]
    k = 21
    ref = sc.count(k, regions, NV, True, 1, -1, 8)
    return k, regions, ref


def test_distinct_counts_and_radix_buckets(genomes):
    k, regions, ref = genomes
    n_ref, buckets_ref = sc.distinct(ref.keys, 16)
    by_build = sc.distinct_by_build(k, regions)
    assert n_ref == len(by_build) < ref.included // 2 and np.array_equal(np.unique(np.array(ref.keys, np.int64)), by_build)
    s = ga.DeviceDbSizer(k, NV, hist_bits=8, radix_bits=16, keep_keys=True)
    _add(s, regions)
    _equal(s.counts(), ref)
    n, buckets = s.distinct()
    assert n == n_ref and np.array_equal(buckets, buckets_ref) and int(buckets.sum()) == n
    assert np.array_equal(buckets, np.bincount(by_build & 0xffff, minlength=1 << 16))
    assert s.distinct()[0] == n  # (asked again: the same answer)
    st = s.stats()
    assert st.n_keys == ref.included and st.n_distinct == n
    assert 16 * ref.included <= st.bytes_peak < 40 * ref.included
    seq, off = sc.pack([r for r, _ in regions])
    assert ga.lib().gs_dbsize_add(s.h, seq.ctypes.data, off.ctypes.data, np.zeros(4, np.int32).ctypes.data, 4, 0) == STATE
    # three planned ranges on the same handle: counts and buckets add up to the one-range result
    max_pairs = next(m for m in range(-(-ref.included // 3), ref.included) if sc.greedy_ranges(ref.hist, m) == 3)
    ranges = ga.plan_ranges(ref.hist, 8, k, max_pairs)
    assert len(ranges) == 3
    total, acc = 0, np.zeros(1 << 16, np.int64)
    for lo, hi in ranges:
        s.set_range(lo, hi)
        _add(s, regions, per_region=True)
        n_r, b_r = s.distinct()
        assert n_r == sc.distinct([x for x in ref.keys if lo <= x < hi])[0] > 0
        _equal(s.counts(), ref)  # (the range restricts only what is retained)
        total += n_r
        acc += b_r
    assert total == n and np.array_equal(acc, buckets)
    s.close()


def test_a_counting_handle_refuses_distinct(genomes):
    k, regions, ref = genomes
    s = ga.DeviceDbSizer(k, NV, hist_bits=8, radix_bits=16)
    _add(s, regions[:1])
    with pytest.raises(ga.GsError) as e:
        s.distinct()
    assert e.value.code == STATE
    assert s.counts()[0].included == ref.per_value[0]
    assert s.stats().bytes_peak == 0
    s.close()
    s = ga.DeviceDbSizer(k, NV, keep_keys=True)  # no radix: the count alone
    _add(s, regions)
    assert s.distinct() == (sc.distinct(ref.keys)[0], None)
    s.close()


def test_the_plan_meets_the_builder(genomes):
    """histogram of fill + update regions -> plan for a third of the k-mers -> gs_dbbuild range by range == the one-shot build"""
    k, regions, _ = genomes
    parent = np.array([-1, 0, 0, 1, 1], np.int32)
    fill, update = regions[:2], regions[2:]
    s = ga.DeviceDbSizer(k, NV, hist_bits=10)
    _add(s, fill)
    h_fill = s.counts()[2]
    s.set_range(0, 1 << (2 * k))
    _add(s, update)
    h_upd = s.counts()[2]
    s.close()
    hist = h_fill + h_upd  # histograms are additive
    ref = sc.count(k, regions, NV, True, 1, -1, 10)
    assert np.array_equal(hist, ref.hist)
    max_pairs = ref.included // 3
    ranges = ga.plan_ranges(hist, 10, k, max_pairs)
    assert len(ranges) >= 3 and ranges[0][0] == 0 and ranges[-1][1] == 1 << (2 * k)
    keys = np.array(ref.keys, np.int64)
    for lo, hi in ranges:
        in_range = int(np.count_nonzero((keys >= lo) & (keys < hi)))
        assert in_range == int(hist[lo >> (2 * k - 10):hi >> (2 * k - 10)].sum()) <= max_pairs

    def build(lo=None, hi=None):
        b = ga.DeviceDbBuilder(k, NV, parent)
        if lo is not None:
            b.set_range(lo, hi)
        for part, upd in ((fill, False), (update, True)):
            seq, off = sc.pack([r for r, _ in part])
            b.add(seq, off, np.array([t for _, t in part], np.int32), update=upd)
        out = b.finish()
        b.close()
        return out

    whole = build()
    parts = [build(lo, hi) for lo, hi in ranges]
    assert len(whole[0]) > 0 and all(len(p[0]) <= max_pairs for p in parts)
    assert np.array_equal(np.concatenate([p[0] for p in parts]), whole[0])
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
