"""Deterministic synthetic workloads shared by tests and bench.py.

Not part of the hot path: it only manufactures inputs -- a k-mer store with a small taxonomy (the same
arrays a Java host would hand over through KMerStore.visit) and fixed-length reads (libgssynth.so, the same
bytes on the host and directly in HBM).

Store recipe: tree root -> G genera -> S species each; every species gets a random genome of `genome_len`
bases (splitmix64-seeded), 5 % of it copied from its genus core and 1 % from a root core, so that k-mers
shared inside a genus / across genera exist; each canonical k-mer is stored with the LCA of the species
containing it (mirrors FillDBGoal + DBGoal's LCA update, C/goals/refseq/DBGoal.java:233-256).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SYN = None
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _splitmix64(state, n):
    """n outputs of splitmix64 starting from `state` (numpy, vectorised via the counter form)"""
    idx = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(state) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _random_dna(state, n):
    return _ACGT[(_splitmix64(state, n) >> np.uint64(33)) & np.uint64(3)]


def canonical_kmers(seq, k):
    """canonical k-mers (reference encoding, CGAT.java:66-74,145-147) of every window of an ACGT byte array"""
    lut = np.zeros(256, dtype=np.uint64)
    for ch, v in zip(b"CGAT", range(4)):
        lut[ch] = v
    c = lut[seq]
    n = len(seq) - k + 1
    fwd = np.zeros(n, dtype=np.uint64)
    rev = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | c[j:j + n]
        rev = rev | ((c[j:j + n] ^ np.uint64(1)) << np.uint64(2 * j))
    return np.maximum(fwd, rev).astype(np.int64)


class SynthDB:
    """arrays of a synthetic store: kmers (sorted int64), value_idx, parent_vi, genomes (S_total x genome_len)"""

    def __init__(self, k=31, genera=4, species_per_genus=5, genome_len=100_000, seed=42, native=True, build=True):
        """build=False: tree and genomes only (the store is then built from the genomes on the device, gs_dbbuild)"""
        self.k, self.genome_len = k, genome_len
        n_species = genera * species_per_genus
        # value indices in pre-order: root 0, genus, its species, next genus ...
        parent, genus_vi, species_vi, taxids = [-1], [], [], ["1"]
        vi = 1
        for g in range(genera):
            genus_vi.append(vi)
            parent.append(0)
            taxids.append(str(1000 + g))
            vi += 1
            for s in range(species_per_genus):
                species_vi.append(vi)
                parent.append(genus_vi[g])
                taxids.append(str(100000 + g * 1000 + s))
                vi += 1
        self.n_values = vi
        self.parent_vi = np.array(parent, dtype=np.int32)
        self.taxids = taxids
        self.species_vi = np.array(species_vi, dtype=np.int32)
        root_core = _random_dna(seed * 1000003 + 1, genome_len)
        genomes = np.empty((n_species, genome_len), dtype=np.uint8)
        seg = 500  # shared material is copied in 500-base segments
        n_seg = genome_len // seg
        # the shared segments are the same for every member of a genus (5 %) / for every species (1 %)
        root_pick = (_splitmix64(seed * 7 + 1, n_seg) % np.uint64(100)) < np.uint64(1)
        covered = n_seg * seg
        root_rep = np.repeat(root_pick, seg)
        for g in range(genera):
            genus_core = _random_dna(seed * 1000003 + 100 + g, genome_len)
            genus_pick = (_splitmix64(seed * 7 + 100 + g, n_seg) % np.uint64(100)) < np.uint64(5)
            # (a root segment wins over a genus segment)
            shared = np.where(root_rep, root_core[:covered], genus_core[:covered])
            is_shared = root_rep | np.repeat(genus_pick, seg)
            for s in range(species_per_genus):
                i = g * species_per_genus + s
                gen = _random_dna(seed * 1000003 + 10000 + i, genome_len)
                genomes[i] = gen
                genomes[i, :covered] = np.where(is_shared, shared, gen[:covered])
        self.genomes = genomes
        self.kmers, self.value_idx = (_build_native if native else _build_numpy)(genomes, k, self.species_vi, self.parent_vi) if build else (None, None)

    @property
    def n_entries(self):
        return len(self.kmers)


def _build_numpy(genomes, k, species_vi, parent_vi):
    """k-mer -> LCA of the species containing it (reference implementation of the recipe; the default is the same in
    C++ on all cores, _build_native)"""
    ks, vs = [], []
    for i in range(len(genomes)):
        u = np.unique(canonical_kmers(genomes[i], k))
        ks.append(u)
        vs.append(np.full(len(u), species_vi[i], dtype=np.int32))
    allk = np.concatenate(ks)
    allv = np.concatenate(vs)
    order = np.argsort(allk, kind="stable")
    allk, allv = allk[order], allv[order]
    first = np.concatenate([[True], allk[1:] != allk[:-1]])
    starts = np.flatnonzero(first)
    par = parent_vi
    vmin = np.minimum.reduceat(allv, starts)
    vmax = np.maximum.reduceat(allv, starts)
    gmin, gmax = par[vmin], par[vmax]  # genus of the smallest / largest species (pre-order => contiguous)
    val = np.where(vmin == vmax, vmin, np.where(gmin == gmax, gmin, 0)).astype(np.int32)
    return allk[first], val


def _build_native(genomes, k, species_vi, parent_vi):
    genomes = np.ascontiguousarray(genomes, dtype=np.uint8)
    sv = np.ascontiguousarray(species_vi, dtype=np.int32)
    pv = np.ascontiguousarray(parent_vi, dtype=np.int32)
    n = C.c_int64(0)
    h = _syn().gs_synth_db_build(genomes.ctypes.data_as(C.c_void_p), genomes.shape[0], genomes.shape[1], k,
                                 sv.ctypes.data_as(C.c_void_p), pv.ctypes.data_as(C.c_void_p), C.byref(n))
    if not h:
        raise MemoryError("gs_synth_db_build failed")
    kmers = np.empty(n.value, dtype=np.int64)
    vals = np.empty(n.value, dtype=np.int32)
    _syn().gs_synth_db_fetch(h, kmers.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p))
    return kmers, vals


def _syn():
    global _SYN
    if _SYN is None:
        path = os.path.join(_HERE, "libgssynth.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: build with `make -C genestrip_amd/csrc`")
        from .binding import _preload_hip_runtime
        _preload_hip_runtime()
        L = C.CDLL(path)
        args = [C.c_uint64, C.c_uint64, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.gs_synth_reads_host.restype, L.gs_synth_reads_host.argtypes = None, args
        L.gs_synth_reads_device.restype, L.gs_synth_reads_device.argtypes = C.c_int, args
        L.gs_synth_db_build.restype = C.c_void_p
        L.gs_synth_db_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gs_synth_db_fetch.restype, L.gs_synth_db_fetch.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p]
        bargs = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
        L.gs_synth_bloom_xor_host.restype, L.gs_synth_bloom_xor_host.argtypes = None, bargs
        L.gs_synth_bloom_xor_device.restype, L.gs_synth_bloom_xor_device.argtypes = C.c_int, bargs
        _SYN = L
    return _SYN


def reads_host(genomes, n_reads, read_len=150, seed=4242, first=0):
    """(seq uint8[n*L], offsets uint64[n+1]) on the host"""
    genomes = np.ascontiguousarray(genomes, dtype=np.uint8)
    seq = np.empty(n_reads * read_len, dtype=np.uint8)
    off = np.empty(n_reads + 1, dtype=np.uint64)
    _syn().gs_synth_reads_host(seed, first, n_reads, read_len, genomes.ctypes.data_as(C.c_void_p), genomes.shape[0],
                               genomes.shape[1], seq.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p))
    return seq, off


def reads_device(genomes_dev, n_genomes, genome_len, n_reads, seq_dev, off_dev, read_len=150, seed=4242, first=0):
    """fill device buffers (tensor-likes with data_ptr()) with the same reads as reads_host"""
    rc = _syn().gs_synth_reads_device(seed, first, n_reads, read_len, C.c_void_p(genomes_dev.data_ptr()), n_genomes,
                                      genome_len, C.c_void_p(seq_dev.data_ptr()), C.c_void_p(off_dev.data_ptr()))
    if rc != 0:
        raise RuntimeError(f"gs_synth_reads_device failed: hip error {-rc}")


# ---------------------------------------------------------------------------------------------------------------
# Index filter inputs (the arrays a Java host hands to gs_bloom_create: AbstractKMerBloomFilter fields bits, hashes,
# hashFactors, bitVector).  Manufactured here, independently of the CPU oracle, so that the filter workloads at
# BASELINE.json configs[2] scale do not depend on test infrastructure; tests/test_synth_cpu.py compares both.
# ---------------------------------------------------------------------------------------------------------------
def java_random_longs(seed, n):
    """first n values of new java.util.Random(seed).nextLong()"""
    mask = (1 << 48) - 1
    s = (seed ^ 0x5DEECE66D) & mask
    out = []

    def nxt(bits):
        nonlocal s
        s = (s * 0x5DEECE66D + 0xB) & mask
        v = s >> (48 - bits)
        return v - (1 << bits) if v >= 1 << (bits - 1) else v  # (int) cast

    for _ in range(n):
        v = ((nxt(32) << 32) + nxt(32)) & ((1 << 64) - 1)
        out.append(v - (1 << 64) if v >= 1 << 63 else v)
    return np.array(out, dtype=np.int64)


def xor_bloom_geometry(expected_insertions, fpp):
    """(bits, hashes, hash_factors) of an XORKMerBloomFilter sized for `expected_insertions` keys at `fpp`
    (AbstractKMerBloomFilter.java:172-185; factors :105-109 from Random(42))"""
    import math
    n = int(expected_insertions)
    bits = max(1, int(-n * math.log(fpp) / (math.log(2.0) * math.log(2.0))))
    hashes = max(1, int(math.floor(bits / n * math.log(2.0) + 0.5)))
    return bits, hashes, java_random_longs(42, hashes)


def xor_bloom_host(keys, bits, factors):
    """bit array (uint64 words) of the filter after putLong of every key"""
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    factors = np.ascontiguousarray(factors, dtype=np.int64)
    words = np.zeros((bits + 63) // 64, dtype=np.uint64)
    _syn().gs_synth_bloom_xor_host(keys.ctypes.data_as(C.c_void_p), len(keys), bits, factors.ctypes.data_as(C.c_void_p),
                                   len(factors), words.ctypes.data_as(C.c_void_p))
    return words


def xor_bloom_device(keys_dev, n_keys, bits, factors_dev, n_hashes, words_dev):
    """the same on the GPU: keys_dev int64[n_keys], factors_dev int64[n_hashes], words_dev zeroed int64[(bits+63)//64]"""
    rc = _syn().gs_synth_bloom_xor_device(C.c_void_p(keys_dev.data_ptr()), n_keys, bits, C.c_void_p(factors_dev.data_ptr()),
                                          n_hashes, C.c_void_p(words_dev.data_ptr()))
    if rc != 0:
        raise RuntimeError(f"gs_synth_bloom_xor_device failed: hip error {-rc}")


# ---------------------------------------------------------------------------------------------------------------
# Skewed workloads: what real samples do to the match path and uniform random genomes do not -- large shared fractions,
# low-complexity sequence, near-identical strains, one genome taking almost every read, reads that hit nothing, ragged
# lengths with N runs, lower case and exact duplicates.  Pure numpy and seeded; the store itself is built from `regions()`
# by the caller (the tests use the oracle's DBGoal restatement).
# ---------------------------------------------------------------------------------------------------------------
_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b


def _low_complexity(rng, n):
    """n bases of homopolymers, short tandem repeats and two-letter islands"""
    out = np.empty(n, dtype=np.uint8)
    i = 0
    while i < n:
        kind = int(rng.integers(0, 3))
        m = min(n - i, int(rng.integers(20, 300)))
        if kind == 0:
            out[i:i + m] = _ACGT[int(rng.integers(0, 4))]
        elif kind == 1:
            unit = _ACGT[rng.integers(0, 4, int(rng.integers(2, 7)))]
            out[i:i + m] = np.resize(unit, m)
        else:
            out[i:i + m] = _ACGT[rng.choice(4, 2, replace=False)][rng.integers(0, 2, m)]
        i += m
    return out


def _with_islands(rng, seq, frac):
    """at least `frac` of the bases of `seq` (in place) overwritten by low-complexity islands of 100 .. 600 bases: (seq, mask)"""
    n = len(seq)
    mask = np.zeros(n, dtype=bool)
    while mask.sum() < frac * n:
        m = int(rng.integers(100, 600))
        p = int(rng.integers(0, max(1, n - m)))
        seq[p:p + m] = _low_complexity(rng, min(m, n - p))
        mask[p:p + m] = True
    return seq, mask


class SkewedDB:
    """a root / genus / species tree over value indices with genomes:
      - each species genome: 20 .. 30 % genus-shared, 5 % root-shared (1 kb segments), >= 6 % low-complexity islands;
      - `strains` near-identical strains (species of genus 0, copies of its first species with <= 1 % of the bases changed);
      - one small `dominant` genome (species, random, unshared) whose value index is the last one, n_values - 1;
      - `n_values` (if larger than the tree needs) padded with genome-less nodes under the genera, placed before the species.
    Parents precede children.  regions() -> (seq, offsets, node_vi) of the genomes, for FillDBGoal / DBGoal."""

    def __init__(self, genera=3, species_per_genus=4, genome_len=150_000, strains=2, dominant_len=2000, n_values=0, seed=1):
        rng = np.random.default_rng(seed)
        n_species = genera * species_per_genus + strains
        need = 1 + genera + n_species + 1
        pad = max(0, n_values - need)
        self.n_values = need + pad
        parent = [-1] + [0] * genera
        parent += [1 + int(x) for x in rng.integers(0, genera, pad)]  # padding nodes, no genome
        first_species = len(parent)
        species_genus = [g for g in range(genera) for _ in range(species_per_genus)] + [0] * strains
        parent += [1 + g for g in species_genus]
        self.dominant_vi = len(parent)
        parent.append(1 + genera - 1)
        self.parent_vi = np.array(parent, dtype=np.int32)
        self.genus_vi = np.arange(1, 1 + genera, dtype=np.int32)
        self.species_vi = np.arange(first_species, first_species + n_species, dtype=np.int32)
        self.strain_vi = self.species_vi[genera * species_per_genus:]
        seg = 1000
        n_seg = genome_len // seg
        root_core, root_lc = _with_islands(rng, _ACGT[rng.integers(0, 4, genome_len)], 0.06)
        genus_core, genus_lc = zip(*[_with_islands(rng, _ACGT[rng.integers(0, 4, genome_len)], 0.06) for _ in range(genera)])
        # which 1 kb segments are shared: the same for every member of a genus / for every species
        seg_kind = np.zeros(n_seg, dtype=np.int8)
        seg_kind[rng.choice(n_seg, max(1, round(n_seg / 20)), replace=False)] = 2  # root 5 %
        genus_seg = []
        for g in range(genera):
            kind = seg_kind.copy()
            free = np.flatnonzero(kind == 0)
            kind[rng.choice(free, int(n_seg * rng.uniform(0.21, 0.29)), replace=False)] = 1
            genus_seg.append(np.repeat(kind, seg))
        genomes, self.low_complexity, self.shared = [], [], []  # (per genome: masks of low-complexity / genus-shared / root-shared bases)
        for i, g in enumerate(species_genus[:genera * species_per_genus]):
            gen, lc = _with_islands(rng, _ACGT[rng.integers(0, 4, genome_len)], 0.07)
            kind = np.zeros(genome_len, dtype=np.int8)
            kind[:len(genus_seg[g])] = genus_seg[g]
            gen = np.where(kind == 2, root_core, np.where(kind == 1, genus_core[g], gen))
            self.low_complexity.append(np.where(kind == 2, root_lc, np.where(kind == 1, genus_lc[g], lc)))
            self.shared.append(kind)
            genomes.append(gen)
        for _ in range(strains):  # near-identical strains of the first species: 0.5 % of the bases substituted
            gen = genomes[0].copy()
            pos = rng.choice(genome_len, genome_len // 200, replace=False)
            gen[pos] = _ACGT[(np.searchsorted(_ACGT, gen[pos]) + rng.integers(1, 4, len(pos))) % 4]
            genomes.append(gen)
            self.low_complexity.append(self.low_complexity[0])
            self.shared.append(self.shared[0])
        genomes.append(_ACGT[rng.integers(0, 4, dominant_len)])
        self.low_complexity.append(np.zeros(dominant_len, dtype=bool))
        self.shared.append(np.zeros(dominant_len, dtype=np.int8))
        self.genomes = genomes
        self.genome_vi = np.concatenate([self.species_vi, [self.dominant_vi]]).astype(np.int32)

    def regions(self):
        """(seq, offsets, node_vi): one region per genome"""
        off = np.concatenate([[0], np.cumsum([len(g) for g in self.genomes])]).astype(np.uint64)
        return np.concatenate(self.genomes), off, self.genome_vi.copy()


def _revcomp(b):
    return _COMP[b[::-1]]


def skewed_reads(db, n_reads, mix, seed=0, cuts=(), sub_rate=0.002):
    """reads of one mix, drawn from `seed`: (seq uint8, offsets uint64[n+1], info dict of per-read arrays)
      dominated:  90 % of the reads from db's dominant genome, the rest from the other genomes, 150 bp;
      background: 95 % random reads (no k-mer in the store), 150 bp;
      ragged:     lengths 35 .. 151, about 10 % at 152 .. 450; 2 % with N runs of 1 .. 40 bases, 2 % with a lower-case stretch;
                  about 5 % exact duplicates of earlier reads, among them the first reads behind every index in `cuts`
                  (batch / shard boundaries), duplicates of reads just in front of it;
      combined:   a third of each, in that order.
    Every read of a genome comes from a random position and strand, with `sub_rate` substitutions per base.
    info: src (genome index, -1 = random), pos, length, clean (unchanged genome text of that strand), dup_of (-1 or the read it
    copies), has_n, lower."""
    if mix == "combined":
        a, b = n_reads // 3, n_reads // 3
        parts = [skewed_reads(db, a, "dominated", seed * 3 + 1, (), sub_rate),
                 skewed_reads(db, b, "background", seed * 3 + 2, (), sub_rate),
                 skewed_reads(db, n_reads - a - b, "ragged", seed * 3 + 3, [c - a - b for c in cuts if c > a + b], sub_rate)]
        lens = np.concatenate([np.diff(p[1].astype(np.int64)) for p in parts])
        info = {key: np.concatenate([p[2][key] for p in parts]) for key in parts[0][2]}
        for lo, hi in ((0, a), (a, a + b), (a + b, n_reads)):  # dup_of indices into the whole batch
            d = info["dup_of"][lo:hi]
            d[d >= 0] += lo
        return np.concatenate([p[0] for p in parts]), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), info
    rng = np.random.default_rng([seed, {"dominated": 1, "background": 2, "ragged": 3}[mix]])
    n_gen = len(db.genomes)
    dom = n_gen - 1
    if mix == "dominated":
        src = np.where(rng.random(n_reads) < 0.9, dom, rng.integers(0, n_gen - 1, n_reads))
        length = np.full(n_reads, 150)
    elif mix == "background":
        src = np.where(rng.random(n_reads) < 0.95, -1, rng.integers(0, n_gen - 1, n_reads))
        length = np.full(n_reads, 150)
    elif mix == "ragged":
        src = rng.integers(0, n_gen, n_reads)
        src[src == dom] = 0
        length = np.where(rng.random(n_reads) < 0.1, rng.integers(152, 451, n_reads), rng.integers(35, 152, n_reads))
    else:
        raise ValueError(mix)
    glen = np.array([len(g) for g in db.genomes])
    length = np.where(src >= 0, np.minimum(length, glen[np.maximum(src, 0)]), length)
    pos = np.where(src >= 0, (rng.random(n_reads) * (glen[np.maximum(src, 0)] - length + 1)).astype(np.int64), 0)
    strand = rng.random(n_reads) < 0.5
    off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    seq = _ACGT[rng.integers(0, 4, int(off[-1]))]  # (random reads keep these bases)
    for gi in range(n_gen):
        idx = np.flatnonzero(src == gi)
        if idx.size == 0:
            continue
        g = db.genomes[gi]
        L = length[idx]
        # for every base of these reads: its genome position and its place in the batch
        tot = int(L.sum())
        rel = np.arange(tot) - np.repeat(np.cumsum(L) - L, L)
        gpos = np.repeat(pos[idx], L) + rel
        dst = np.repeat(off[idx], L) + rel
        seq[dst] = g[gpos]
    for r in np.flatnonzero(strand & (src >= 0)):
        seq[off[r]:off[r + 1]] = _revcomp(seq[off[r]:off[r + 1]])
    clean = src >= 0
    # substitutions
    hit = np.flatnonzero(rng.random(len(seq)) < sub_rate)
    seq[hit] = _ACGT[(np.searchsorted(_ACGT, seq[hit]) + rng.integers(1, 4, len(hit))) % 4]
    read_of = np.searchsorted(off, hit, side="right") - 1
    clean[read_of] = False
    has_n = np.zeros(n_reads, dtype=bool)
    lower = np.zeros(n_reads, dtype=bool)
    dup_of = np.full(n_reads, -1, dtype=np.int64)
    if mix == "ragged":
        for r in rng.choice(n_reads, max(1, n_reads // 50), replace=False):
            L = int(length[r])
            m = min(L, int(rng.integers(1, 41)))
            p = int(rng.integers(0, L - m + 1))
            seq[off[r] + p:off[r] + p + m] = ord("N")
            has_n[r] = True
        for r in rng.choice(n_reads, max(1, n_reads // 50), replace=False):
            L = int(length[r])
            m = min(L, int(rng.integers(1, 30)))
            p = int(rng.integers(0, L - m + 1))
            seq[off[r] + p:off[r] + p + m] += 32  # (N becomes n)
            lower[r] = True
        clean &= ~has_n & ~lower
        # exact duplicates: ~5 % of the reads copy an earlier read (the lengths change, so the batch is rebuilt)
        dups = set(rng.choice(np.arange(1, n_reads), max(1, n_reads // 20), replace=False).tolist())
        for c in cuts:
            for j in range(3):
                if 3 <= c + j < n_reads:
                    dups.add(c + j)
                    dup_of[c + j] = c - 1 - j
        for r in sorted(dups):
            if dup_of[r] < 0:
                dup_of[r] = int(rng.integers(max(0, r - 5000), r))
        reads = [seq[off[r]:off[r + 1]] for r in range(n_reads)]
        for r in np.flatnonzero(dup_of >= 0):  # in read order, so that a copy of a copy is the same text
            reads[r] = reads[dup_of[r]]
            for arr in (src, pos, length, clean, has_n, lower):
                arr[r] = arr[dup_of[r]]
        length = np.array([len(x) for x in reads])
        off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
        seq = np.concatenate(reads) if reads else np.zeros(0, np.uint8)
    info = dict(src=src.astype(np.int64), pos=pos.astype(np.int64), length=length.astype(np.int64), clean=clean, strand=strand,
                dup_of=dup_of, has_n=has_n, lower=lower)
    return np.ascontiguousarray(seq, dtype=np.uint8), off.astype(np.uint64), info


def fastq_text(seq, offsets, names=None):
    """four-line FASTQ of the reads: descriptor '@' + names[i] (default b"r<i>"), the read, '+', quality 'I' x length"""
    off = offsets.astype(np.int64)
    out = []
    for i in range(len(off) - 1):
        s = seq[off[i]:off[i + 1]].tobytes()
        out.append(b"@" + (names[i] if names is not None else b"r%d" % i) + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
    return b"".join(out)
