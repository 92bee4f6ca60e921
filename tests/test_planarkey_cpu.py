"""tests/planarkey.py (the store's key scheme restated from the comments of gs_layout.h) against the CPU oracle's canonical
k-mers, against itself (mix / unmix, scalar / numpy forms) and, for the placement rule, against hand-made key lists."""
import numpy as np
import pytest

import planarkey as pk
from oracle import gs_oracle as orc

KS = (1, 5, 15, 18, 19, 21, 22, 30, 31)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _revcomp(s):
    return s.translate(COMP)[::-1]


def _kmers(k, n, seed):
    """n random k-mers plus, at even k, reverse-complement palindromes; the homopolymers and two alternating ones on top"""
    rng = np.random.default_rng(seed)
    out = [bytes(x) for x in np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, k))]]
    if k % 2 == 0:
        for _ in range(max(4, n // 10)):
            half = bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, k // 2)])
            out.append(half + _revcomp(half))
            assert out[-1] == _revcomp(out[-1])
    out += [bytes([c]) * k for c in b"ACGT"] + [(b"AC" * k)[:k], (b"GT" * k)[:k]]
    return out


@pytest.mark.parametrize("k", KS)
def test_key_round_trip_is_the_oracles_canonical_kmer(k):
    for s in _kmers(k, 300, 100 + k):
        h = pk.key(s)
        assert 0 <= h < 1 << pk.KEY_BITS
        assert h == pk.key(_revcomp(s)) == pk.key(s.lower())
        hi, lo = pk.unmix(h)
        assert hi >> k == 0 and lo >> k == 0
        assert (hi, lo) == pk.rep(*pk.planes(s), k) == pk.rep(*pk.planes(_revcomp(s)), k)
        want = orc.kmer_canonical(s, 0, k)
        assert pk.kmer_of_planes(hi, lo, k) == want == pk.kmer_of_planes(*pk.planes(s), k)
        assert pk.bases_of_planes(hi, lo, k) in (s, _revcomp(s))
        # the planes of the reference value, read in either orientation, lead to the same key
        assert pk.mix(*pk.rep(*pk.planes_of_kmer(want, k), k)) == h


@pytest.mark.parametrize("k", [k for k in KS if k >= 15])
def test_distinct_kmers_have_distinct_keys(k):
    rng = np.random.default_rng(k)
    x = rng.integers(0, 1 << 62, 110_000, dtype=np.int64) & ((1 << (2 * k)) - 1)
    seq = np.frombuffer(b"CGAT", dtype=np.uint8)[(x[:, None] >> (2 * (k - 1 - np.arange(k)))) & 3]
    canon = np.unique(np.array([orc.kmer_canonical(bytes(r), 0, k) for r in seq[:2000]], dtype=np.int64))
    # (the oracle's canonical value for a sample; the vector form below, held to it, for all of them)
    hi, lo = pk.planes_of_kmers_np(x, k)
    rhi, rlo = pk.rep_np(hi, lo, k)
    keys = pk.mix_np(rhi, rlo)
    for i in range(0, 2000, 7):
        assert int(keys[i]) == pk.key(bytes(seq[i]))
        assert pk.kmer_of_planes(int(rhi[i]), int(rlo[i]), k) == orc.kmer_canonical(bytes(seq[i]), 0, k)
    assert len(canon) > 1900
    # distinct canonical k-mers = distinct representative plane pairs (one per strand class)
    pairs = np.unique((rhi << np.uint64(32)) | rlo)
    pairs = pairs[:100_000]
    assert len(pairs) == 100_000
    keys = pk.mix_np(pairs >> np.uint64(32), pairs & np.uint64(0xffffffff))
    assert len(np.unique(keys)) == 100_000
    assert int(keys.max()) < 1 << pk.KEY_BITS
    a, b = pk.unmix_np(keys)
    assert np.array_equal(a, pairs >> np.uint64(32)) and np.array_equal(b, pairs & np.uint64(0xffffffff))
    back = pk.kmers_of_planes_np(a, b, k)
    assert len(np.unique(back)) == 100_000
    assert back[:300].tolist() == [pk.kmer_of_planes(int(x), int(y), k) for x, y in zip(a[:300], b[:300])]
    wk, valid = pk.window_keys_np(seq[:50].reshape(-1), k)  # windows over a concatenation: every k-th is one of the k-mers
    assert valid.all() and np.array_equal(wk[::k], pk.keys_of_kmers_np(x[:50], k))


def test_mix_is_a_bijection_on_plane_pairs():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 1 << 31, 20000, dtype=np.int64)
    b = rng.integers(0, 1 << 31, 20000, dtype=np.int64)
    edge = [0, 1, (1 << 31) - 1, 1 << 30, 0x55555555 & ((1 << 31) - 1)]
    pairs = [(x, y) for x in edge for y in edge] + list(zip(a.tolist(), b.tolist()))
    hs = pk.mix_np([p[0] for p in pairs], [p[1] for p in pairs])
    for (x, y), h in zip(pairs[:3000], hs[:3000].tolist()):
        assert pk.mix(x, y) == h < 1 << pk.KEY_BITS
        assert pk.unmix(h) == (x, y)
    for h in (0, 1, 2, (1 << 62) - 1, 1 << 31, (1 << 31) - 1, 1 << 40):
        assert pk.mix(*pk.unmix(h)) == h
    assert len(np.unique(hs)) == len(set(pairs))


def test_owner_is_taken_above_bit_40():
    for h, world, want in ((0, 3, 0), ((1 << 40) - 1, 3, 0), (1 << 40, 3, 1), (5 << 40, 3, 2), (((1 << 22) - 1) << 40, 64, 63),
                           ((7 << 40) | 12345, 1, 0)):
        assert pk.owner(h, world) == want


def test_window_keys_mark_every_window_with_a_foreign_byte():
    seq = np.frombuffer(b"ACGTNacgtACGTRACGTACGTACGT", dtype=np.uint8)
    for k in (1, 4, 5):
        for alphabet in (b"ACGT", b"ACGTacgt"):  # the matcher's alphabet (a lower-case base is foreign, as for the oracle), and both cases
            keys, valid = pk.window_keys_np(seq, k, alphabet)
            for p in range(len(seq) - k + 1):
                w = bytes(seq[p:p + k])
                ok = all(c in alphabet for c in w)
                assert bool(valid[p]) == ok
                if alphabet == b"ACGT":
                    assert ok == (orc.kmer_straight(w, 0, k)[1] == -1)
                if ok:
                    assert int(keys[p]) == pk.key(w)
    assert len(pk.window_keys_np(seq[:3], 4)[0]) == 0


def _check_placement(keys, values, b, slots, max_disp, vbits):
    """every key is where a probe finds it, and a displaced entry stands only behind full buckets"""
    mask = (1 << b) - 1
    table = slots.reshape(-1, pk.SLOTS)
    full = (table != 0).all(axis=1)
    where = {}
    for bk in range(1 << b):
        row = table[bk]
        n = int((row != 0).sum())
        assert (row[:n] != 0).all() and (row[n:] == 0).all()  # filled from slot 0 on
        for s in row[:n].tolist():
            rem, disp, v, seen = pk.slot_fields(s, vbits)
            home = (bk - disp) & mask
            assert seen == 0 and all(full[(home + d) & mask] for d in range(disp))
            where[(rem << b) | home] = (v, disp)
    assert len(where) == len(keys)
    assert all(where[h][0] == v for h, v in zip(keys, values))
    assert max_disp == max([d for _, d in where.values()], default=0)
    return where


def test_place_displaces_only_behind_full_buckets():
    vbits, b0 = pk.value_bits(5)
    assert (vbits, b0) == (3, 4)
    key_at = lambda home, rem: (rem << 4) | home
    # bucket 5 full, a ninth key of home 5 goes to bucket 6 with displacement 1
    keys = [key_at(5, r) for r in range(1, 10)]
    values = [i % 5 for i in range(len(keys))]
    b, slots, md = pk.place(keys, values, b0, 6.0, vbits)
    w = _check_placement(keys, values, b, slots, md, vbits)
    assert (b, md) == (4, 1) and w[keys[8]] == (values[8], 1) and all(w[h][1] == 0 for h in keys[:8])
    # buckets 6 and 7 filled by their own keys (6 holds the displaced one already): the next key of home 5 lands in bucket 8 with 3
    keys += [key_at(6, r) for r in range(1, 8)] + [key_at(7, r) for r in range(1, 9)] + [key_at(5, 100)]
    values = [i % 5 for i in range(len(keys))]
    b, slots, md = pk.place(keys, values, b0, 6.0, vbits)
    w = _check_placement(keys, values, b, slots, md, vbits)
    assert (b, md) == (4, 3) and w[keys[-1]][1] == 3
    assert pk.slot_fields(int(slots[8 * pk.SLOTS]), vbits) == (100, 3, values[-1], 0)
    assert pk.displaced_share(slots, vbits) == 2 / len(keys)
    # the order decides: with the key of home 5 placed before bucket 7 fills, it takes a slot there with displacement 2
    early = keys[:-9] + [keys[-1]] + keys[-9:-1]
    b, slots, md = pk.place(early, values, b0, 6.0, vbits)
    w = _check_placement(early, values, b, slots, md, vbits)
    assert w[keys[-1]][1] == 2 and md == 2 and w[keys[-2]][1] == 1  # ... and the last key of home 7 is pushed on to bucket 8
    # wrap-around: home 15 full, the next goes to bucket 0
    wrap = [key_at(15, r) for r in range(1, 10)]
    b, slots, md = pk.place(wrap, [0] * 9, b0, 6.0, vbits)
    _check_placement(wrap, [0] * 9, b, slots, md, vbits)
    assert (b, md) == (4, 1) and pk.slot_fields(int(slots[0]), vbits) == (9, 1, 0, 0)
    # no place within three buckets: the table doubles and starts again (33 keys of one home at b = 4; at b = 5 they split by bit 4)
    many = [key_at(5, r) for r in range(1, 34)]
    b, slots, md = pk.place(many, [1] * 33, b0, 6.0, vbits)
    _check_placement(many, [1] * 33, b, slots, md, vbits)
    assert b == 5 and md == 2  # homes 5 (rem even: 16 keys) and 21 (17 keys)
    # the starting size: the smallest b >= b0 with 2^b * load >= n
    assert pk.place(list(range(97)), [0] * 97, b0, 6.0, vbits)[0] == 5
    assert pk.place(list(range(96)), [0] * 96, b0, 6.0, vbits)[0] == 4
    assert pk.place(list(range(49)), [0] * 49, b0, 3.0, vbits)[0] == 5
    assert pk.place([], [], b0, 3.0, vbits)[0] == 4
