"""gs_filter_kernel (gs_filter.hip) at every hash count, fill, k, read length, threshold and filter geometry, byte for byte against
the oracle's FastqBloomFilter.isAcceptRead (orc.Bloom.filter_batch) or, for filters of 2^31 .. 2^37 bits, the sparse host
reference (tests/bloomref.py SparseBloom).  Every cell asserts with the host reference that its edge happened.

Kernel branch                                               cells that take it
----------------------------------------------------------  ------------------------------------------------------------
n_hashes 1-3: the `nh <= S` shortcut, no batching           staging/{xor,murmur}/h{1,2,3}/{sparse,dense}, geometry/*/{1,2}
n_hashes 4-6: idle lanes t >= T masked in pass4             staging/*/h{4,5,6}/*, geometry/* (5 hashes), text/xor-h5-k16
n_hashes 7: T = 4, first slice empty                        staging/*/h7/*, lengths, k/* (fpp 0.01)
n_hashes 8-14: first slice partly used (lane < 8 && i < nh) staging/*/h{8,11,14}/*, factors/* (8 hashes)
n_hashes 15: first slice exactly full                       staging/*/h15/*
n_hashes 16-64: the tail loop                               staging/*/h{16,17,40,64}/*, thresholds (20 hashes)
several fkey batches, short last batch (4 * nb mask)        staging/*/h>=4/dense (asserted: > 16 survivors, short batch;
                                                            key 0 is a member, so a phantom idle group would count)
fcand filled from several batches                           staging/*/h>=7/dense (asserted: nc_max)
false candidates in the first slice / the tail loop         staging/*/h>=8/dense, h>=16/dense (asserted)
round 0: sampled pass, second pass, later rounds            thresholds/* (asserted: `need` reached in each)
early exit (members >= need)                                thresholds/*, staging/* (adaptive min_pos)
need = max((int)(max * ratio), 1) in double                 thresholds/* (reads at need - 1, need, need + 1; (max, ratio)
                                                            pairs where float32, ceil and round give another need)
blocked path (start, start + 1 + (uh >> 60))                blocked/* (asserted: members whose second word is start + 16)
magic division, shift == 0 (bits = 1)                       geometry/*/1, also bits 2, 2^j +- 1, primes
magic division at INT64_MIN, +-(2^63 - 1), multiples +- 1   factors/*
32-bit word / byte offsets (2^31 .. 2^37 bits)              huge/* (device-built; neighbours at +- 2^30 .. 2^36)
text mode (records found on the device), CRLF               text/*
k = 1 .. 31, even-k palindromes; k = 0 / 32 refused         k/*, test_filter_k_refused

Needs an MI355X: run with -m gpu."""
import math
import time

import numpy as np
import pytest

import bloomref as br
import genestrip_amd as ga
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

HASHES = (1, 2, 3, 4, 5, 6, 7, 8, 11, 14, 15, 16, 17, 40, 64)  # tests/test_filter_ref_cpu.py asserts fpp -> n_hashes
STAGING_N = 2000
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _dna(rng, n):
    return bytes(rng.choice(ACGT, n))


def _device(ob):
    return ga.DeviceBloomFilter(ob.kind, ob.bits, ob.hash_factors, ob.words, n_hashes=max(ob.hashes, 1))


def _check(ob, k, thresholds, reads):
    """every threshold's accept bytes, device vs oracle; -> the oracle's accept arrays"""
    seq, off = orc.pack_reads(reads)
    gb = _device(ob)
    wants = []
    try:
        for mp, ratio in thresholds:
            got = ga.FastqBloomFilter(k, gb, mp, ratio).accept_reads(seq, off)
            want = ob.filter_batch(k, mp, ratio, seq, off, threads=4)
            assert np.array_equal(got, want), (k, mp, ratio, np.flatnonzero(got != want)[:10])
            wants.append(want)
    finally:
        gb.close()
    return wants


def _hb(ob, k, reads):
    """per read: (hash bits [max, n_hashes], valid [max]) from the host reference"""
    words, factors = ob.words, ob.hash_factors
    out = []
    for r in reads:
        keys, valid = br.read_keys(r, k)
        out.append((br.hash_bits(ob.kind, factors, ob.bits, words, keys), valid))
    return out


def _members(hbv):
    return np.array([int((hb.all(axis=1) & v).sum()) for hb, v in hbv])


def _random_words(rng, bits, density):
    nw = (bits + 63) // 64
    return np.packbits(rng.random((nw, 64)) < density, axis=1, bitorder="little").view(np.uint64).reshape(nw)


# ------------------------------------------------------------------ staging: every hash count, sparse and near-saturated
def _staging_reads(rng, genome):
    reads = []
    lengths = [150] * 4 + [250, 250, 31, 38, 95, 159]
    for i in range(360):
        L = lengths[i % len(lengths)]
        kind = i % 3
        if kind == 0:  # from the member genome, a few substitutions
            p = int(rng.integers(0, len(genome) - L))
            r = bytearray(genome[p:p + L])
            for q in rng.integers(0, L, int(rng.integers(0, 4))):
                r[q] = int(rng.choice(ACGT))
        elif kind == 1:
            r = bytearray(_dna(rng, L))
        else:  # a member window inside random bases
            r = bytearray(_dna(rng, L))
            w = int(rng.integers(31, L + 1))
            p, o = int(rng.integers(0, len(genome) - w)), int(rng.integers(0, L - w + 1))
            r[o:o + w] = genome[p:p + w]
        if i % 17 == 0:
            r[int(rng.integers(0, L))] = ord("N") if i % 2 else ord("a")
        reads.append(bytes(r))
    return reads


@pytest.mark.parametrize("fill", ["sparse", "dense"])
@pytest.mark.parametrize("h", HASHES)
@pytest.mark.parametrize("kind", [orc.BLOOM_XOR, orc.BLOOM_MURMUR], ids=["xor", "murmur"])
def test_filter_staging(kind, h, fill):
    rng = np.random.default_rng(1000 * h + 10 * kind + (fill == "dense"))
    geo = orc.Bloom(kind, STAGING_N, br.fpp_for_hashes(h))
    assert geo.hashes == h
    bits, factors = geo.bits, geo.hash_factors
    genome = _dna(rng, STAGING_N + 30)
    keys = orc.canonical_kmers(genome, 31)
    if fill == "sparse":  # every 20th k-mer: ~3 % of the bits set
        ob = orc.Bloom.raw(kind, bits, h, factors)
        ob.put_many(keys[::20])
    else:  # 95 % of the bits set, every k-mer of the genome, and key 0, which no read has (C..C is read as G..G)
        ob = orc.Bloom.raw(kind, bits, h, factors, _random_words(rng, bits, 0.95))
        ob.put_many(keys)
        ob.put(0)
        assert ob.contains(0)
    reads = _staging_reads(rng, genome)
    hbv = _hb(ob, 31, reads)
    counts = _members(hbv)
    qs = sorted({max(int(q), 2) for q in np.percentile(counts[counts > 0], [25, 50, 75])})
    thresholds = [(1, 0.2), (0, 0.5)] + [(q, 0.2) for q in qs]
    wants = _check(ob, 31, thresholds, reads)
    assert any(0 < w.sum() < len(w) for w in wants)
    hb_all = np.concatenate([hb for hb, _ in hbv])
    valid_all = np.concatenate([v for _, v in hbv])
    s3 = hb_all[:, :min(3, h)].all(axis=1) & valid_all & ~hb_all.all(axis=1)
    if fill == "sparse":  # almost no non-member survives hashes 0-2 (~3 % of the bits are set)
        assert s3.mean() < (0.05 if h == 1 else 0.01)
        return
    # premises of the near-saturated filter: several batches, a short last batch, a full fcand, false candidates
    need = max(qs)
    tr = [br.stage_trace(hb, v, need) for hb, v in hbv if len(v)]
    if h > 3:
        assert max(t["s1_max"] for t in tr) > 16
        assert any(t["short_batch"] for t in tr)
    if h >= 7:
        assert max(t["nc_max"] for t in tr) >= 40
    if h >= 8:
        assert any(t["slice_fail"] for t in tr)
    if h >= 16:
        assert any(t["tail_fail"] for t in tr)
    # a kernel that skipped hash 2 (h >= 3), 14 (h >= 15) or 15 (h >= 16) would answer differently on some read
    for skip in [i for i in (2, 14, 15) if i < h]:
        keep = np.ones(h, dtype=bool)
        keep[skip] = False
        flips = 0
        for (mp, ratio), w in zip(thresholds, wants):
            for (hb, v), r, a in zip(hbv, reads, w):
                m = int((hb[:, keep].all(axis=1) & v).sum())
                flips += (len(v) > 0 and m >= br.need_of(len(v), mp, ratio)) != bool(a)
        assert flips > 0, skip


# ------------------------------------------------------------------ k
def _palindrome(rng, k):
    half = rng.choice(ACGT, k // 2)
    comp = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}
    return bytes(half) + bytes(comp[c] for c in reversed(half.tolist()))


K_CELLS = [(orc.BLOOM_XOR, k) for k in (1, 2, 8, 14, 15, 16, 20, 24, 30, 31)] + \
          [(orc.BLOOM_MURMUR, k) for k in (2, 8, 16, 24)] + [(orc.BLOOM_BLOCKED, k) for k in (1, 8, 16, 24)]


@pytest.mark.parametrize("kind,k", K_CELLS, ids=["%s/k%d" % ("xor murmur blocked".split()[c], k) for c, k in K_CELLS])
def test_filter_k(kind, k):
    rng = np.random.default_rng(77 + k + 100 * kind)
    genome = _dna(rng, 600)
    keys = np.unique(orc.canonical_kmers(genome, k))
    keys = rng.permutation(keys)[: max(len(keys) // 2, 1)]
    pals = [_palindrome(rng, k) for _ in range(8)] if k % 2 == 0 else []
    ob = orc.Bloom(kind, max(len(keys), 1), 0.01)
    assert kind == orc.BLOOM_BLOCKED or ob.hashes == (7 if len(keys) >= 50 else ob.hashes)  # fpp 0.01: 7 hashes
    ob.put_many(keys)
    for p in pals[:4]:
        ob.put(orc.kmer_canonical(p))
    reads = []
    for i in range(400):
        L = int(rng.integers(0, 300))
        if i % 2:
            p = int(rng.integers(0, len(genome) - min(L, 599)))
            r = bytearray(genome[p:p + L])
        else:
            r = bytearray(_dna(rng, L))
        if pals and L >= k and i % 4 < 2:
            o = int(rng.integers(0, L - k + 1))
            r[o:o + k] = pals[i % len(pals)]
        if i % 11 == 0 and L:
            r[int(rng.integers(0, L))] = ord("n")
        reads.append(bytes(r))
    wants = _check(ob, k, [(1, 0.2), (0, 0.5), (3, 0.0), (0, 0.0)], reads)
    assert all(0 < w.sum() < len(w) for w in wants[:1])
    if pals:  # reverse-complement palindromes: forward == reverse, in the reads and in the filter
        for p in pals:
            assert orc.kmer_straight(p, 0, k)[0] == orc.kmer_reverse(p, 0, k)[0]
        assert any(ob.contains(orc.kmer_canonical(p)) for p in pals)


def test_filter_k_refused():
    ob = orc.Bloom(orc.BLOOM_XOR, 100, 0.01)
    gb = _device(ob)
    seq, off = orc.pack_reads([b"ACGT" * 10])
    try:
        for k in (0, 32, -1):
            with pytest.raises(ga.GsError):
                ga.FastqBloomFilter(k, gb, 1, 0.2).accept_reads(seq, off)
        assert ga.FastqBloomFilter(31, gb, 1, 0.2).accept_reads(seq, off).tolist() == [0]  # the handle still works
    finally:
        gb.close()


# ------------------------------------------------------------------ read lengths
def test_filter_read_lengths():
    """max = 1 .. 129 around the 64-position rounds, reads of 10^4 .. 10^6 bases, members only in the last round, odd bytes"""
    rng = np.random.default_rng(31)
    genome = _dna(rng, 4000)
    keys = orc.canonical_kmers(genome, 31)
    ob = orc.Bloom(orc.BLOOM_XOR, len(keys), 0.01)
    assert ob.hashes == 7
    ob.put_many(keys)
    reads, last_only = [], []
    for mx in (1, 7, 8, 9, 63, 64, 65, 127, 128, 129):
        L = mx + 30
        for j in range(12):
            r = bytearray(_dna(rng, L))
            if j % 3 == 0:  # members only in the last round
                w = int(rng.integers(1, mx - 64 * ((mx - 1) // 64) + 1))
                p = int(rng.integers(0, len(genome) - w - 30))
                r[L - w - 30:] = genome[p:p + w + 30]
                last_only.append(len(reads))
            elif j % 3 == 1:
                p = int(rng.integers(0, len(genome) - L))
                r[:] = genome[p:p + L]
            if j >= 9 and j % 3:
                r[int(rng.integers(0, L))] = [0, ord("U"), ord("-"), 0xFF, ord("\r"), ord("c")][j % 6]
            reads.append(bytes(r))
    for L in (10_000, 100_000, 1_000_000):
        r = bytearray(_dna(rng, L))
        for o in rng.integers(0, L - 200, 5):
            p = int(rng.integers(0, len(genome) - 60))
            r[o:o + 60] = genome[p:p + 60]
        r[int(rng.integers(0, L))] = ord("N")
        reads.append(bytes(r))
        r = bytearray(_dna(rng, L))  # one member run at the very end
        p = int(rng.integers(0, len(genome) - 40))
        r[L - 40:] = genome[p:p + 40]
        last_only.append(len(reads))
        reads.append(bytes(r))
    for i in last_only:  # an N on every false positive of the random bases before the last round (it ends those windows)
        r = bytearray(reads[i])
        (hb, v), = _hb(ob, 31, [reads[i]])
        for q in np.flatnonzero(hb.all(axis=1) & v):
            if q < 64 * ((len(v) - 1) // 64):
                r[q] = ord("N")
        reads[i] = bytes(r)
    wants = _check(ob, 31, [(1, 0.2), (0, 0.0), (0, 0.5), (2, 0.0), (0, 1e-5)], reads)
    hbv = _hb(ob, 31, reads)
    for i in last_only:  # premise: the read's members all sit in its last round, and it is accepted
        hb, v = hbv[i]
        mpos = np.flatnonzero(hb.all(axis=1) & v)
        assert len(mpos) and mpos.min() >= 64 * ((len(v) - 1) // 64), i
        assert wants[0][i] == 1
    assert any(br.stage_trace(*hbv[i], 1)["reached"] == "later" for i in last_only)


# ------------------------------------------------------------------ thresholds
def _need_pairs():
    """(max, ratio) pairs where the double product truncates to another integer than the float32 product (the first three: the
    double product lies just below an integer, so ceil and round differ too), or lies just above an integer (ceil differs)"""
    f32, above = [], []
    for mx in range(20, 300):
        for c in range(1, 100):
            ratio = c / 100.0
            d = int(float(mx) * ratio)
            f = int(np.float32(mx) * np.float32(ratio))
            if f > d and len(f32) < 3 and d >= 2:
                f32.append((mx, ratio))
            x = float(mx) * ratio
            if x != math.floor(x) and x - math.floor(x) < 1e-9 and len(above) < 2 and d >= 2:
                above.append((mx, ratio))
    assert len(f32) == 3 and len(above) == 2
    return f32 + above


def test_filter_thresholds():
    """reads with exactly need - 1, need and need + 1 member positions at every kind of need, built from member runs in random
    bases (20 hashes, fpp 1e-6: the runs' edges are no members); the reference decides and the premises are checked with it"""
    rng = np.random.default_rng(8)
    genome = _dna(rng, 20000)
    keys = orc.canonical_kmers(genome, 31)
    ob = orc.Bloom(orc.BLOOM_XOR, len(keys), 1e-6)
    assert ob.hashes == 20
    ob.put_many(keys)
    pairs = _need_pairs()
    # (max, min_pos, ratio, run offset): need reached in round 0's sampled pass (runs from 0, need <= 8), its second pass
    # (runs from 1, no multiple of 8 before need), a later round (runs from 64)
    configs = [(120, 5, 0.2, 0), (120, 8, 0.2, 0), (120, 5, 0.2, 1), (120, 0, 0.25, 1), (120, 0, 0.25, 70), (120, 0, 0.0, 64),
               (200, 0, 0.1, 130), (120, 121, 0.2, 0), (64, 64, 0.0, 0)] + [(mx, 0, r, 0) for mx, r in pairs] + \
              [(mx, 0, r, mx % 64) for mx, r in pairs]
    # runs from 0 whose sampled positions (0, 8, ..) alone reach need, or fall one short of it
    configs = [c + (None,) for c in configs] + [(120, 8, 0.0, 0, (64, 57, 56)), (120, 2, 0.0, 0, (9, 8)), (120, 9, 0.0, 0, (64,))]
    results = []
    for mx, mp, ratio, o, run_lengths in configs:
        need = br.need_of(mx, mp, ratio)
        reads, ms = [], []
        for m in run_lengths or (need - 1, need, need + 1):
            m = min(m, mx)
            if m < 0:
                continue
            oo = min(o, mx - m)
            r = bytearray(_dna(rng, mx + 30))
            if m:  # the bases around the run differ from the genome's, so the run has exactly m member positions
                p = int(rng.integers(1, len(genome) - m - 31))
                r[oo:oo + m + 30] = genome[p:p + m + 30]
                if oo > 0:
                    r[oo - 1] = b"CA"[genome[p - 1] == ord("C")]
                if oo + m + 30 < len(r):
                    r[oo + m + 30] = b"CA"[genome[p + m + 30] == ord("C")]
            reads.append(bytes(r))
            ms.append(m)
        want = _check(ob, 31, [(mp, ratio)], reads)[0]
        hbv = _hb(ob, 31, reads)
        assert _members(hbv).tolist() == ms, (mx, mp, ratio)
        assert want.tolist() == [int(m >= need) for m in ms]
        results += [br.stage_trace(hb, v, need)["reached"] for hb, v in hbv]
        if (mx, ratio) in pairs[:3]:  # float32, ceil and round ask for another need
            x = float(mx) * ratio
            assert need not in (int(np.float32(mx) * np.float32(ratio)), math.ceil(x), round(x))
        if (mx, ratio) in pairs[3:]:
            assert math.ceil(float(mx) * ratio) != need
    assert {"r0p0", "r0p1", "later"} <= set(results)


# ------------------------------------------------------------------ geometry: bits, magic divisors, hash factors
GEOMETRY = [1, 2, 63, 64, 65, 127, 129, 8191, 65537, 999983, 1000003, (1 << 24) - 1, (1 << 24) + 1]


@pytest.mark.parametrize("bits", GEOMETRY)
@pytest.mark.parametrize("kind", [orc.BLOOM_XOR, orc.BLOOM_MURMUR], ids=["xor", "murmur"])
def test_filter_geometry(kind, bits):
    rng = np.random.default_rng(bits + kind)
    h = 2 if bits <= 2 else 5
    ob = orc.Bloom.raw(kind, bits, h, rng.integers(-(1 << 63), (1 << 63) - 1, h, dtype=np.int64, endpoint=True),
                       None if bits <= 2 else _random_words(rng, bits, 0.5))
    genome = _dna(rng, 3000)
    if bits > 2:
        ob.put_many(orc.canonical_kmers(genome, 31)[: max(bits // 8, 10)])
    reads = [genome[i:i + 40 + i % 50] for i in range(0, 2900, 23)] + [_dna(rng, 40 + i % 90) for i in range(150)]
    wants = _check(ob, 31, [(1, 0.2), (0, 0.3), (0, 0.8)], reads)
    assert ob.bits == bits and len(ob.words) == (bits + 63) // 64
    if bits > 2:
        assert any(0 < w.sum() < len(w) for w in wants)
    # bits <= 2 with nothing put: no member; then every bit set: every valid k-mer is one
    if bits <= 2:
        assert not any(w.any() for w in wants)
        ob.put(1)
        ob.put(2)
        assert ob.words[0] == (1 << bits) - 1
        wants = _check(ob, 31, [(1, 0.2), (0, 1.0)], reads)
        assert all(w.all() for w in wants)


@pytest.mark.parametrize("bits", [1000003, (1 << 20) + 1, 1 << 20, 4099])
@pytest.mark.parametrize("kind", [orc.BLOOM_XOR, orc.BLOOM_MURMUR], ids=["xor", "murmur"])
def test_filter_hash_factor_edges(kind, bits):
    """factors chosen so that the hashed value of a read's k-mer is INT64_MIN, +-(2^63 - 1) or a multiple of bits +- 1 (XOR:
    factor ^ key; Murmur: the same factors, hashed values elsewhere)"""
    rng = np.random.default_rng(bits)
    genome = _dna(rng, 400)
    keys = orc.canonical_kmers(genome, 31)
    m = ((1 << 62) // bits) * bits
    targets = [-(1 << 63), (1 << 63) - 1, -(1 << 63) + 1, m + 1, m - 1, -(m + 1), -m, m]
    sel = keys[:: len(keys) // len(targets)][: len(targets)]
    factors = np.array([int(key) ^ t for key, t in zip(sel.tolist(), targets)], dtype=np.int64)
    ob = orc.Bloom.raw(kind, bits, len(targets), factors)
    ob.put_many(sel)
    reads = [genome[i:i + 31] for i in range(0, 370)] + [_dna(rng, 31) for _ in range(200)] + [genome]
    _check(ob, 31, [(1, 0.2), (0, 0.5)], reads)
    if kind == orc.BLOOM_XOR:
        hv = br.hash_values(kind, factors, sel)
        assert [int(hv[i, i]) for i in range(len(targets))] == targets
        idx = br.hash_index(kind, factors, bits, sel)
        assert idx[6, 6] == 0 and idx[3, 3] == 1 and idx[4, 4] == bits - 1
    assert all(ob.contains(x) for x in sel.tolist())


# ------------------------------------------------------------------ blocked
@pytest.mark.parametrize("k,buckets,long_len", [(15, 1, 10_000), (21, None, 100_000), (31, 1000003, 20_000), (8, 3, 5000)])
def test_filter_blocked(k, buckets, long_len):
    rng = np.random.default_rng(k)
    genome = _dna(rng, 5000)
    keys = np.unique(orc.canonical_kmers(genome, k))
    if buckets is None:
        ob = orc.Bloom(orc.BLOOM_BLOCKED, len(keys), 0.01)
    else:  # a seed under which some keys have their second word at start + 16 (short keys leave the top bits to the seed)
        while True:
            seed = int(rng.integers(-(1 << 62), 1 << 62))
            s1, s2, _, _ = br.blocked_probe(seed, buckets, keys)
            if ((s2 - s1) == 16).sum() >= 3:
                break
        ob = orc.Bloom.raw(orc.BLOOM_BLOCKED, buckets, 0, [seed])
    assert len(ob.words) == ob.bits + 17
    seed = int(ob.hash_factors[0])
    s1, s2, _, _ = br.blocked_probe(seed, ob.bits, keys)
    far = keys[(s2 - s1) == 16]  # second word at start + 16
    ob.put_many(keys[::3] if ob.bits > 64 else keys[:2])  # a few keys only where there are a few words
    ob.put_many(far if ob.bits > 64 else far[:2])
    reads = [genome[i:i + k] for i in range(0, 4900, 7)]
    reads += [bytes(_dna(rng, k)) for _ in range(300)]
    reads += [genome[i:i + 150] for i in range(0, 4800, 97)]
    r = bytearray(_dna(rng, long_len))
    r[long_len // 2:long_len // 2 + 200] = genome[:200]
    reads.append(bytes(r))
    wants = _check(ob, k, [(1, 0.2), (0, 0.5), (0, 0.0)], reads)
    assert 0 < wants[0].sum() < len(reads)
    far = far[br.blocked_contains(seed, ob.bits, ob.words, far)]
    on_reads = set(far.tolist()) & {orc.kmer_canonical(r) for r in reads[:700]}
    assert on_reads, "no single-k-mer read holds a member whose second word is start + 16"
    if buckets == 1:
        assert len(ob.words) == 18


# ------------------------------------------------------------------ text mode
def _fastq(reads, nl):
    return b"".join(b"@r%d" % i + nl + r + nl + b"+" + nl + b"I" * len(r) + nl for i, r in enumerate(reads))


TEXT_CELLS = [("xor-h15-dense", orc.BLOOM_XOR, 15, 31), ("murmur-h40-dense", orc.BLOOM_MURMUR, 40, 31),
              ("xor-h5-k16", orc.BLOOM_XOR, 5, 16), ("blocked-1bucket-k15", orc.BLOOM_BLOCKED, 0, 15)]


@pytest.mark.parametrize("name,kind,h,k", TEXT_CELLS, ids=[c[0] for c in TEXT_CELLS])
def test_filter_text_mode(name, kind, h, k):
    rng = np.random.default_rng(h + k)
    genome = _dna(rng, 3000)
    keys = orc.canonical_kmers(genome, k)
    if kind == orc.BLOOM_BLOCKED:
        ob = orc.Bloom.raw(kind, 1, 0, [12345])
        ob.put_many(keys[::40])
    else:
        geo = orc.Bloom(kind, STAGING_N, br.fpp_for_hashes(h))
        ob = orc.Bloom.raw(kind, geo.bits, h, geo.hash_factors, _random_words(rng, geo.bits, 0.95 if h > 5 else 0.02))
        ob.put_many(keys)
    reads = _staging_reads(rng, genome)[:300] + [b"", b"ACG", genome[:k], b"N" * 40]
    lens = [len(r) for r in reads]
    for mp, ratio in ((1, 0.2), (0, 0.5)):
        for nl in (b"\n", b"\r\n"):
            text = _fastq(reads, nl)
            p = orc.parse_fastq(text, k=k)  # '\r' stays in the read, as in the reference's parser
            assert np.diff(p["seq_off"].astype(np.int64)).tolist() == [n + (nl == b"\r\n") for n in lens]
            want = ob.filter_batch(k, mp, ratio, p["seq"] if len(p["seq"]) else np.zeros(1, np.uint8), p["seq_off"])
            gb = _device(ob)
            try:
                f = ga.FastqBloomFilter(k, gb, mp, ratio)
                acc = np.full(len(reads), 7, dtype=np.uint8)
                f.submit_text(text, acc)
                f.sync()
                assert f.text_status()[0] == -1
            finally:
                gb.close()
            assert np.array_equal(acc, want), (nl, mp, np.flatnonzero(acc != want)[:10])
            assert 0 < want.sum() < len(want)


# ------------------------------------------------------------------ 2^31 .. 2^37 bits, built on the device
def _decode(key, k=31):
    return bytes(b"CGAT"[(key >> (2 * (k - 1 - j))) & 3] for j in range(k))


HUGE = [("2^31", (1 << 31) + 1), ("2^32", (1 << 32) + 1), ("2^33", (1 << 33) + 3), ("2^36", (1 << 36) + (1 << 34) + 7)]


@pytest.mark.parametrize("name,target", HUGE, ids=[c[0] for c in HUGE])
def test_filter_huge_geometry(name, target):
    """A 1-hash XOR filter (fpp 0.5) of 2^31 .. 2^37 bits built by gs_bloom_build from a few keys, probed with member reads whose
    bits lie high (above 2^35 and 2^36 in the largest) and with non-member reads whose bit is exactly a member's +- 2^30, 2^31,
    2^32, 2^35 or 2^36: a 32-bit wrap of the word, dword or byte offset, in the probe or in the probe and the builder alike, fails"""
    n = int(math.ceil(target * math.log(2.0)))
    while br.geometry(n, 0.5)[0] < target:
        n += 1
    bits, nh = br.geometry(n, 0.5)
    assert nh == 1 and target <= bits < target + 4 and bits <= 1 << 37
    f0 = orc.JRandom(42).next_long()
    rng = np.random.default_rng(bits & 0xFFFF)
    pool = np.unique(np.concatenate([orc.canonical_kmers(_dna(rng, 2000), 31) for _ in range(4)]))
    pos = br.jabs_mod(pool ^ np.int64(f0), bits)
    bands = [(bits // 2, bits)] + [(1 << j, min(1 << (j + 1), bits)) for j in (30, 31, 32, 35) if (1 << j) < bits // 2]
    members = np.unique(np.concatenate([pool[(pos >= lo) & (pos < hi)][:24] for lo, hi in bands]))
    sp = br.SparseBloom(orc.BLOOM_XOR, bits, [f0])
    for key in members.tolist():
        sp.put(key)
    neighbours = []  # (key, position): position = a member's +- 2^j, whose bit is clear
    for key in members.tolist():
        h = br._signed(f0 ^ key)
        p = abs(h) % bits
        for j in (30, 31, 32, 35, 36):
            for d in ((1 << j), -(1 << j)):
                if not 0 <= p + d < bits:
                    continue
                h2 = h + d if h >= 0 else h - d
                k2 = f0 ^ h2
                if not (-(1 << 63) <= h2 < (1 << 63)) or not 0 <= k2 < (1 << 62):
                    continue
                if orc.kmer_canonical(_decode(k2)) != k2:  # not the canonical orientation of its read
                    continue
                assert sp.positions(k2) == [p + d] and not sp.contains(k2)
                neighbours.append((k2, p + d))
    if bits > (1 << 36):
        assert any(sp.positions(key)[0] >= (1 << 36) for key in members.tolist())
        assert any((1 << 35) <= sp.positions(key)[0] < (1 << 36) for key in members.tolist())
        assert {abs(pp - q) for (_, pp) in neighbours for q in (sp.positions(m)[0] for m in members.tolist())} >= {1 << 35, 1 << 36}
    assert len(neighbours) >= 8
    reads = [_decode(key) for key in members.tolist()] + [_decode(key) for key, _ in neighbours]
    reads.append(b"".join(reads))  # one long read of all of them
    want = np.array([sp.accept(r, 31, 1, 0.2) for r in reads], dtype=np.uint8)
    assert want[:len(members)].all() and not want[len(members):-1].any()
    seq, off = orc.pack_reads(reads)
    t0 = time.perf_counter()
    gb = ga.DeviceBloomFilter.build(members, expected_insertions=n, fpp=0.5)
    try:
        gbits, gf, gw = gb.get(with_words=False)
        assert gbits == bits and gf.tolist() == [f0] and gw is None
        got = ga.FastqBloomFilter(31, gb, 1, 0.2).accept_reads(seq, off)
    finally:
        gb.close()
    dt = time.perf_counter() - t0
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    print("huge %s: %d bits (%.2f GiB on the device), %d members, %d neighbours, %.2f s" %
          (name, bits, bits / 8 / 2**30, len(members), len(neighbours), dt))
