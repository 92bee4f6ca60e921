"""Host references for the read filter's tests (tests/test_gpu_filter_edges.py, tests/test_filter_ref_cpu.py).

* ``hash_index`` / ``hash_bits`` / ``read_keys``: the filters' bit indices (Math.abs(h % bits), XORKMerBloomFilter.java:43-59,
  MurmurKMerBloomFilter) and a read's canonical k-mers in numpy, so a test can see every hash of every position.
* ``SparseBloom``: a filter held as the set of its set words, in Python ints; for filters of 2^31 .. 2^37 bits whose words the
  host never holds.
* ``fpp_for_hashes`` / ``geometry``: the (n, fpp) -> (bits, n_hashes) rule of AbstractKMerBloomFilter (:172-185) and the fpp
  that gives each hash count the tests use.
* ``stage_trace``: what gs_filter_kernel's XOR / Murmur staging meets on one read (survivors of hashes 0-2, batches of 16,
  candidates, the hash a false candidate fails at, where `need` is reached), so each GPU cell can assert that its edge happened.
"""
import math

import numpy as np

BLOOM_XOR, BLOOM_MURMUR, BLOOM_BLOCKED = 0, 1, 2
M64 = (1 << 64) - 1
S_LANE = 3  # gs_filter_kernel: hashes 0..2 per lane, then 4 (T) per survivor, a first slice of 8, the tail
CODES = {ord("C"): 0, ord("G"): 1, ord("A"): 2, ord("T"): 3}  # CGAT.java:66-69; lower case and the rest are invalid


def fpp_for_hashes(h):
    """fpp whose optimal hash count (Math.round(bits / n * ln 2)) is h: bits ~ n * log2(1 / fpp) / ln 2"""
    return 2.0 ** -h


def geometry(n, fpp):
    """AbstractKMerBloomFilter.optimalNumOfBits :183-185 and optimalNumOfHashFunctions :172-174 (as orc_bloom_create and
    gs_bloom_build compute them)"""
    bits = max(int(-n * math.log(fpp) / (math.log(2.0) * math.log(2.0))), 1)
    return bits, max(int(math.floor(bits / n * math.log(2.0) + 0.5)), 1)


# ------------------------------------------------------------------ numpy (vectorised) restatement
def _rotl(x, r):
    return (x << np.uint64(r)) | (x >> np.uint64(64 - r))


def murmur64(data, base):
    """MurmurHash3DropIn.hash64(data, base) (:60-87) on int64 arrays (broadcast)"""
    d = np.asarray(data, dtype=np.int64).view(np.uint64)
    h = np.asarray(base, dtype=np.int64).view(np.uint64)
    d, h = np.broadcast_arrays(d, h)
    kk = d.byteswap()
    kk = kk * np.uint64(0x87c37b91114253d5)
    kk = _rotl(kk, 31) * np.uint64(0x4cf5ad432745937f)
    h = h ^ kk
    h = _rotl(h, 27) * np.uint64(5) + np.uint64(0x52dce729)
    h = h ^ np.uint64(8)
    h = h ^ (h >> np.uint64(33))
    h = h * np.uint64(0xff51afd7ed558ccd)
    h = h ^ (h >> np.uint64(33))
    h = h * np.uint64(0xc4ceb9fe1a85ec53)
    h = h ^ (h >> np.uint64(33))
    return (h ^ d).view(np.int64)


def jabs_mod(h, bits):
    """Math.abs(h % bits): np.fmod truncates as Java's % does; |h % bits| < bits, so the abs never overflows"""
    return np.abs(np.fmod(np.asarray(h, dtype=np.int64), np.int64(bits)))


def hash_values(kind, factors, keys):
    """int64 [len(keys), len(factors)]: the value reduced mod bits for each hash (factor ^ key, or Murmur)"""
    k = np.asarray(keys, dtype=np.int64)[:, None]
    f = np.asarray(factors, dtype=np.int64)[None, :]
    return (f ^ k) if kind == BLOOM_XOR else murmur64(k, f)


def hash_index(kind, factors, bits, keys):
    return jabs_mod(hash_values(kind, factors, keys), bits)


def hash_bits(kind, factors, bits, words, keys):
    """bool [len(keys), n_hashes]: is bit i of each key set (XOR / Murmur)"""
    idx = hash_index(kind, factors, bits, keys)
    w = np.asarray(words, dtype=np.uint64)[idx >> 6]
    return ((w >> (idx & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def blocked_probe(seed, buckets, keys):
    """BlockedKMerBloomFilter.containsLong :181-199 -> (start, second word, m1, m2), numpy"""
    h = np.asarray(keys, dtype=np.int64) ^ np.int64(seed)
    start = jabs_mod(h, buckets)
    uh = h.view(np.uint64)
    uh = uh ^ _rotl(uh, 32)
    sh = uh.view(np.int64)
    one = np.uint64(1)

    def bit(s):
        return one << (s & 63).astype(np.uint64)
    m1 = bit(sh) | bit(sh >> 6)
    m2 = bit(sh >> 12) | bit(sh >> 18)
    return start, start + 1 + (uh >> np.uint64(60)).astype(np.int64), m1, m2


def blocked_contains(seed, buckets, words, keys):
    s1, s2, m1, m2 = blocked_probe(seed, buckets, keys)
    w = np.asarray(words, dtype=np.uint64)
    return ((w[s1] & m1) == m1) & ((w[s2] & m2) == m2)


def read_keys(read, k):
    """(keys int64[max], valid bool[max]) of a read: the canonical key max(fwd, revcomp) (CGAT.java:145-147) at every
    position; a window with a byte outside ACGT is invalid"""
    a = np.frombuffer(bytes(read), dtype=np.uint8)
    n = len(a) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    lut = np.full(256, -1, dtype=np.int64)
    for ch, v in CODES.items():
        lut[ch] = v
    codes = lut[a]
    bad = np.concatenate([[0], np.cumsum(codes < 0)])
    valid = (bad[k:] - bad[:-k]) == 0
    c = np.where(codes < 0, 0, codes).astype(np.uint64)
    fwd = np.zeros(n, dtype=np.uint64)
    rev = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        fwd = (fwd << np.uint64(2)) | c[j:j + n]
        rev = rev | ((c[j:j + n] ^ np.uint64(1)) << np.uint64(2 * j))
    return np.maximum(fwd, rev).astype(np.int64), valid


def need_of(max_, min_pos, ratio):
    """FastqBloomFilter.isAcceptRead :120-161: accept <=> members >= max(threshold, 1), threshold = minPosCount or
    (int) (max * ratio) in double precision"""
    thr = min_pos if min_pos > 0 else int(float(max_) * float(ratio))
    return max(thr, 1)


# ------------------------------------------------------------------ sparse filter in Python ints
def _murmur_int(data, base):
    d, h = data & M64, base & M64
    kk = int.from_bytes(d.to_bytes(8, "little"), "big")
    kk = (kk * 0x87c37b91114253d5) & M64
    kk = ((kk << 31) | (kk >> 33)) & M64
    kk = (kk * 0x4cf5ad432745937f) & M64
    h ^= kk
    h = (((((h << 27) | (h >> 37)) & M64) * 5) + 0x52dce729) & M64
    h ^= 8
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & M64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & M64
    h ^= h >> 33
    r = h ^ d
    return r - (1 << 64) if r >> 63 else r


def _signed(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


class SparseBloom:
    """A filter as {word index: word}: bit i of the filter = bit (i & 63) of word i >> 6.  Math.abs(v % bits) is abs(v) % bits
    in Python ints (Java's % truncates toward zero)."""

    def __init__(self, kind, bits, factors):
        self.kind, self.bits, self.factors = kind, int(bits), [int(f) for f in factors]
        self.words = {}

    def positions(self, key):
        """XOR / Murmur: the bit index of every hash of `key`"""
        key = int(key)
        out = []
        for f in self.factors:
            h = _signed(f ^ key) if self.kind == BLOOM_XOR else _murmur_int(key, f)
            out.append(abs(h) % self.bits)
        return out

    def _blocked(self, key):
        h = _signed(self.factors[0] ^ int(key))
        s1 = abs(h) % self.bits
        uh = h & M64
        uh ^= ((uh << 32) | (uh >> 32)) & M64
        sh = _signed(uh)
        m1 = (1 << (sh & 63)) | (1 << ((sh >> 6) & 63))
        m2 = (1 << ((sh >> 12) & 63)) | (1 << ((sh >> 18) & 63))
        return s1, m1, s1 + 1 + (uh >> 60), m2

    def put(self, key):
        if self.kind == BLOOM_BLOCKED:
            s1, m1, s2, m2 = self._blocked(key)
            self.words[s1] = self.words.get(s1, 0) | m1
            self.words[s2] = self.words.get(s2, 0) | m2
            return
        for p in self.positions(key):
            self.words[p >> 6] = self.words.get(p >> 6, 0) | (1 << (p & 63))

    def contains(self, key):
        if self.kind == BLOOM_BLOCKED:
            s1, m1, s2, m2 = self._blocked(key)
            return (self.words.get(s1, 0) & m1) == m1 and (self.words.get(s2, 0) & m2) == m2
        return all((self.words.get(p >> 6, 0) >> (p & 63)) & 1 for p in self.positions(key))

    def members(self, read, k):
        keys, valid = read_keys(read, k)
        return sum(1 for key, v in zip(keys.tolist(), valid.tolist()) if v and self.contains(key))

    def accept(self, read, k, min_pos, ratio):
        max_ = len(read) - k + 1
        return max_ > 0 and self.members(read, k) >= need_of(max_, min_pos, ratio)


# ------------------------------------------------------------------ what the kernel's staging meets
def stage_trace(hb, valid, need):
    """gs_filter_kernel's XOR / Murmur control flow on one read, on the host: hb = bool [max, n_hashes] (hash bits of every
    position), valid = bool [max].  Round r covers positions 64r .. 64r+63; round 0 makes a pass over every 8th position, then
    one over the rest.  Returns a dict:
      s1_max      most survivors of hashes 0-2 in one pass (> 16: several fkey batches)
      short_batch a pass with more than 16 survivors whose last batch is shorter than 16 (the idle-group mask)
      nc_max      most candidates (passed hashes 3..6) of one pass, i.e. the fill of fcand
      slice_fail  a candidate confirmed false at a hash of the first slice (S+T .. S+T+7)
      tail_fail   a candidate confirmed false in the tail loop (S+T+8 ..)
      reached     where members >= need became true: "r0p0", "r0p1", "later" or None
      members     the members counted (early exit included), accept = members >= need"""
    max_, nh = hb.shape
    T = min(max(nh - S_LANE, 0), 4)
    out = dict(s1_max=0, short_batch=False, nc_max=0, slice_fail=False, tail_fail=False, reached=None, members=0)
    members = 0
    full = hb.all(axis=1) & valid
    pos = np.arange(max_)
    for rnd in range((max_ + 63) // 64):
        if members >= need:
            break
        for ps in ((0, 1) if rnd == 0 else (1,)):
            if members >= need:
                break
            lanes = (pos >= 64 * rnd) & (pos < 64 * rnd + 64) & valid
            if rnd == 0:
                lanes &= ((pos & 7) == 0) == (ps == 0)
            s1 = np.flatnonzero(lanes & hb[:, :min(S_LANE, nh)].all(axis=1))
            out["s1_max"] = max(out["s1_max"], len(s1))
            if nh <= S_LANE:
                members += len(s1)
            else:
                confirmed, nc = 0, 0
                for b0 in range(0, len(s1), 16):
                    if members + confirmed >= need:
                        break
                    batch = s1[b0:b0 + 16]
                    if len(batch) < 16 and b0 > 0:
                        out["short_batch"] = True
                    cand = [p for p in batch if hb[p, S_LANE:S_LANE + T].all()]
                    nc += len(cand)
                    for p in cand:
                        if members + confirmed >= need:
                            break
                        if full[p]:
                            confirmed += 1
                        else:
                            first = int(np.flatnonzero(~hb[p])[0])
                            out["slice_fail" if first < S_LANE + T + 8 else "tail_fail"] = True
                out["nc_max"] = max(out["nc_max"], nc)
                members += confirmed
            if members >= need and out["reached"] is None:
                out["reached"] = ("r0p%d" % ps) if rnd == 0 else "later"
    out["members"] = members
    return out
