"""CPU reference of the sizing pass (gs_dbsize: the reference's fillsize and tempindex walks, C/goals/refseq/FillSizeGoal.java
:80-105 and FillBloomFilterGoal.java:154-195 over AbstractStoreFastaReader.java:87-115) in plain Python, from the unchanged oracle
alone: nothing here calls the library under test.

The window rule: for the bases b[0..len) of a region after the optional upper-casing, the window [s, s + k) counts iff all k
bytes are C, G, A or T and (s + k) % step_size == 0.  A counting window adds one to `total`; if max_dust >= 0 and its score
exceeds max_dust it adds one to `dust` and nothing else; otherwise one to `included`, to per_value[tag of the region] and to
hist[canon >> (2k - hb)], hb = min(hist_bits, 2k), canon = the oracle's canonical k-mer; canon is retained if lo <= canon < hi.

  fib / dust_window   the low-complexity score in its window form (per period 1, 2, 3: fib over the runs of positions whose
                      base equals the base `period` earlier); pinned against oracle.dust_value in tests/test_dbsize_cpu.py
  count               -> Size(total, dust, included, per_value, hist, keys): keys = every retained canon, duplicates included
  distinct            -> (number of distinct keys, bucket sizes by the low radix_bits bits)
  distinct_by_build   the distinct set a second way: the oracle's DbBuild filled with every region under value 0
  greedy_ranges       the plan as a three-line greedy over the bins
"""
import types

import numpy as np

from oracle import gs_oracle as orc

BASES = b"CGAT"


def fib(n):
    """0, 1, 2, 3, 5, 8 ..."""
    a, b = 1, 2
    for _ in range(n - 1):
        a, b = b, a + b
    return a if n > 0 else 0


def dust_window(w):
    """w: the k bases of a window (bytes or str)"""
    w = w.encode() if isinstance(w, str) else bytes(w)
    d = 0
    for p in (1, 2, 3):
        run = 0
        for i in range(len(w) - p):
            if w[i] == w[i + p]:
                run += 1
            else:
                d += fib(run)
                run = 0
        d += fib(run)
    return d


def windows(region, k, lower=True, step=1):
    """the counting windows of one region: (start, the k upper-cased bases)"""
    b = bytes(region)
    if lower:
        b = bytes(c - 32 if c in b"acgt" else c for c in b)
    for s in range(len(b) - k + 1):
        w = b[s:s + k]
        if (s + k) % step == 0 and all(c in BASES for c in w):
            yield s, w


def count(k, regions, n_values=1, lower=True, step=1, max_dust=-1, hist_bits=12, lo=0, hi=1 << 64):
    """regions: list of (bytes, tag)"""
    hb = min(hist_bits, 2 * k)
    out = types.SimpleNamespace(total=0, dust=0, included=0, per_value=np.zeros(n_values, np.int64), hist=np.zeros(1 << hb, np.int64),
                                keys=[])
    for region, tag in regions:
        for _, w in windows(region, k, lower, step):
            out.total += 1
            if max_dust >= 0 and dust_window(w) > max_dust:
                out.dust += 1
                continue
            canon = orc.kmer_canonical(w, 0, k)
            out.included += 1
            out.per_value[tag] += 1
            out.hist[canon >> (2 * k - hb)] += 1
            if lo <= canon < hi:
                out.keys.append(canon)
    return out


def distinct(keys, radix_bits=0):
    u = np.unique(np.asarray(keys, dtype=np.int64))
    buckets = np.bincount(u & ((1 << radix_bits) - 1), minlength=1 << radix_bits).astype(np.int64) if radix_bits else None
    return len(u), buckets


def pack(parts):
    """list of bytes -> (seq uint8, offsets uint64)"""
    seq = np.frombuffer(b"".join(parts), dtype=np.uint8)
    if len(seq) == 0:
        seq = np.zeros(1, dtype=np.uint8)
    return seq, np.cumsum([0] + [len(s) for s in parts]).astype(np.uint64)


def distinct_by_build(k, regions, lower=True, step=1, max_dust=-1):
    """ascending distinct canonical k-mers: DbBuild(...).fill(all regions under value 0); optimize(); fetch()"""
    b = orc.DbBuild(k, 1, np.array([-1], np.int32), lower, step, max_dust)
    seq, off = pack([bytes(r) for r, _ in regions])
    b.fill(seq, off, np.zeros(len(regions), np.int32))
    b.optimize()
    kmers, _ = b.fetch()
    b.close()
    return kmers


def greedy_ranges(hist, max_pairs):
    """number of maximal runs of consecutive bins whose sum stays <= max_pairs (every bin <= max_pairs)"""
    n, s = 1, 0
    for h in hist:
        n, s = (n + 1, h) if s + h > max_pairs else (n, s + h)
    return n
