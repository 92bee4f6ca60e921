"""Constructed reads for the prefilter's decision steps (tests/test_prefilter_steps_cpu.py, tests/test_gpu_prefilter_shapes.py):
background reads in which exactly one chosen sample is in S, the same with an N inside that sample, and the same with earlier
samples replaced by decoys -- 15-mers whose level-one bit is set although they are not in S, so that the exact level is asked
and says no before the planted sample is reached.  numpy only; k = 31, where the samples (17 apart) do not overlap."""
import numpy as np

import prefilter as pf

LETTERS = np.frombuffer(b"CGAT", dtype=np.uint8)  # code 0 .. 3 (tests/prefilter.py)


def l1_table(S):
    """the level-one bit table of S: bit ((canon * 0x9E3779B1) mod 2^32) >> 8"""
    t = np.zeros(1 << 24, dtype=bool)
    t[((np.asarray(S, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)] = True
    return t


def l1_bits(canon):
    return (((np.asarray(canon, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)).astype(np.int64)


def lmer_of_code(code):
    """the 15 bytes of the strand whose value (hi << 15 | lo) is `code`"""
    code = int(code)
    hi, lo = code >> 15, code & 0x7FFF
    return LETTERS[[(((hi >> i) & 1) << 1) | ((lo >> i) & 1) for i in range(pf.LMER)]]


def decoys(S, rng, draws=100_000):
    """(n, 15) bytes: random 15-mers with the level-one bit set that are not in S"""
    codes = rng.integers(0, 4, (draws, pf.LMER))
    canon = pf.canon_of_codes(codes)
    keep = l1_table(S)[l1_bits(canon)] & ~np.isin(canon, S)
    return LETTERS[codes[keep]]


def deciding_sample_reads(S, L, k, seed):
    """-> (reads (n, L), expect (n,) bool, decider (n,), decoys (n,)): for every sample index i a background read with a 15-mer of S planted at
    sample i (passes, decided by i), the same read with an N inside the planted sample (rejected), and the same read with two to
    four earlier samples (as many as there are) replaced by decoys (passes, decided by i after the exact level said no);
    decoys = how many decoys a read holds"""
    rng = np.random.default_rng(seed)
    w, pos = pf.stride(k), pf.sample_positions(L, k)
    assert w >= pf.LMER, "the samples must not overlap"
    dec = decoys(S, rng)
    assert len(dec) >= 100, len(dec)
    table = l1_table(S)
    reads, expect, decider, planted = [], [], [], []
    for i, p in enumerate(pos):
        while True:  # a background read none of whose samples passes level one
            base = pf.ACGT[rng.integers(0, 4, L)]
            canon, _ = pf.sample_codes(base[None, :], L, k)
            if not table[l1_bits(canon[0])].any():
                break
        plain = base.copy()
        plain[p:p + pf.LMER] = lmer_of_code(S[int(rng.integers(0, len(S)))])
        with_n = plain.copy()
        with_n[p + int(rng.integers(0, pf.LMER))] = ord("N")
        led = plain.copy()
        at = rng.choice(i, size=min(i, int(rng.integers(2, 5))), replace=False) if i else []
        for j in at:
            led[pos[j]:pos[j] + pf.LMER] = dec[int(rng.integers(0, len(dec)))]
        planted += [0, 0, len(at)]
        reads += [plain, with_n, led]
        expect += [True, False, True]
        decider += [i, -1, i]
    reads = np.ascontiguousarray(np.stack(reads), dtype=np.uint8)
    expect = np.array(expect)
    canon, bad = pf.sample_codes(reads, L, k)
    in_s = np.isin(canon, S) & ~bad
    assert np.array_equal(in_s.any(axis=1), expect) and np.array_equal(pf.passes(S, reads, L, k), expect)
    for r, d in enumerate(decider):  # the planted sample is the only one in S
        assert in_s[r].sum() == (1 if d >= 0 else 0) and (d < 0 or in_s[r, d])
    return reads, expect, np.array(decider), np.array(planted)
