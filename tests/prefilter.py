"""Plain restatement of the sampled 15-mer prefilter (genestrip_amd/csrc/gs_prefilter.h), numpy only.

A stored k-mer at read position s owns the w = k - 14 15-mer positions s .. s + w - 1; exactly one of them is a multiple of w, and
it is <= L - 15.  S = the canonical 15-mers of every stored k-mer.  A read passes iff one of its samples (positions 0, w, 2 w, ..
<= L - 15) is free of bytes that are no upper-case C, G, A, T and lies in S.  A read that holds a stored
k-mer passes; nothing else is promised.
Canonical code of a 15-mer: codes C 0, G 1, A 2, T 3; plane hi / lo = bit 1 / bit 0 of the codes, base i in bit i; a strand's value
is hi << 15 | lo, the reverse complement's the same of the reversed bases with code ^ 1; the smaller of the two is the code."""
import numpy as np

LMER = 15
_CODE = np.full(256, -1, dtype=np.int64)
for _i, _c in enumerate(b"CGAT"):
    _CODE[_c] = _i


def stride(k):
    return k - (LMER - 1)


def sample_positions(L, k):
    return list(range(0, L - LMER + 1, stride(k)))


def canon_of_codes(codes):
    """codes: (n, 15) array of 0 .. 3 -> (n,) canonical codes (30 bits)"""
    codes = np.asarray(codes, dtype=np.int64)
    sh = np.arange(LMER, dtype=np.int64)
    def value(c):
        return (((c >> 1) << sh).sum(axis=1) << LMER) | ((c & 1) << sh).sum(axis=1)
    return np.minimum(value(codes), value(codes[:, ::-1] ^ 1))


def lmer_set(kmers, k):
    """the canonical 15-mers of stored k-mers given in the reference's encoding (two bits per base, first base in the top bits)"""
    kmers = np.asarray(kmers).astype(np.uint64)
    codes = np.stack([((kmers >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)).astype(np.int64) for i in range(k)], axis=1)
    parts = [canon_of_codes(codes[:, d:d + LMER]) for d in range(k - LMER + 1)]
    return np.unique(np.concatenate(parts))


def sample_codes(reads, L, k):
    """reads: (n, L) bytes -> (canon (n, m), bad (n, m)): the code of every sample (arbitrary where bad) and whether it holds a byte
    that is no base"""
    reads = np.asarray(reads, dtype=np.uint8).reshape(-1, L)
    pos = sample_positions(L, k)
    canon = np.zeros((len(reads), len(pos)), dtype=np.int64)
    bad = np.zeros((len(reads), len(pos)), dtype=bool)
    for j, p in enumerate(pos):
        c = _CODE[reads[:, p:p + LMER]]
        bad[:, j] = (c < 0).any(axis=1)
        canon[:, j] = canon_of_codes(np.where(c < 0, 0, c))
    return canon, bad


def passes(S, reads, L, k):
    canon, bad = sample_codes(reads, L, k)
    return (np.isin(canon, S) & ~bad).any(axis=1)


ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def make_reads(genomes, L, k, n, seed):
    """n reads of L bytes: three in four from the genomes (every second of those reverse-complemented, ~1 % substitutions), the rest
    uniform background; then N, lower-case letters and CR bytes sprinkled over a third of all reads.  The first two reads are a
    genome read whose only clean k-mer starts at 0 and one whose only clean k-mer starts at L - k (an N in every other window)"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, genomes.shape[0], n)
    p = rng.integers(0, genomes.shape[1] - L + 1, n)
    seq = np.ascontiguousarray(genomes[g[:, None], p[:, None] + np.arange(L)[None, :]], dtype=np.uint8)
    rc = np.arange(n) % 2 == 1
    seq[rc] = COMP[seq[rc][:, ::-1]]
    sub = rng.random((n, L)) < 0.01
    sub[:2] = False
    seq[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    bg = np.arange(n) % 4 == 3
    seq[bg] = ACGT[rng.integers(0, 4, (int(bg.sum()), L))]
    dirty = np.flatnonzero(rng.random(n) < 0.33)
    dirty = dirty[dirty >= 2]
    for r in dirty:
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, L))
            kind = int(rng.integers(0, 3))
            seq[r, at] = ord("N") if kind == 0 else (seq[r, at] | 0x20 if kind == 1 else 13)
    seq[0, k::k - 1] = ord("N")           # windows 1 .. : each holds an N; window 0 is bases 0 .. k - 1
    seq[1, L - k - 1::-(k - 1)] = ord("N")  # windows .. L - k - 1 likewise; window L - k is clean
    return seq
