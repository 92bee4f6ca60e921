// gs_absmod.h -- the Bloom filters' bit index Math.abs(v % bits) (C/bloom/XORKMerBloomFilter.java:57-59) by a magic-number
// division, shared by the host (gs_api.cpp makes the magic, g++ checks it in tests/native/absmod_check.cpp), the filter kernel and
// the index kernel (gs_index.hip); and the Murmur hash those two kernels share.
#pragma once
#include <stdint.h>

#include "gs_layout.h"

// high 64 bits of the 128-bit product a * b
GS_HD uint64_t gs_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// magic for unsigned division of any 64-bit n by a constant 1 <= d <= 2^63 (round-up method with an add step):
//   l = smallest l with 2^l >= d, magic = floor(2^64 * (2^l - d) / d) + 1, t = mulhi(n, magic),
//   q = (t + ((n - t) >> 1)) >> (l - 1)          (shift = l; shift == 0 <=> d == 1).  Host only (128-bit division).
static inline void gs_magic_u64(uint64_t d, uint64_t &magic, int &shift) {
    int l = 0;
    while (l < 64 && ((uint64_t)1 << l) < d) l++;
    const unsigned __int128 num = ((unsigned __int128)((l == 64 ? 0 : ((uint64_t)1 << l)) - d)) << 64;
    magic = (uint64_t)(num / d) + 1;
    shift = l;
}

// MurmurKMerBloomFilter.hash: MurmurHash3DropIn.hash64(data, base) (C/util/MurmurHash3DropIn.java:60-87)
GS_HD int64_t gs_murmur64(int64_t data_, int64_t base) {
    const uint64_t data = (uint64_t)data_;
    uint64_t hash = (uint64_t)base;
    uint64_t kk = __builtin_bswap64(data);
    kk *= 0x87c37b91114253d5ULL;
    kk = (kk << 31) | (kk >> 33);
    kk *= 0x4cf5ad432745937fULL;
    hash ^= kk;
    hash = ((hash << 27) | (hash >> 37)) * 5 + 0x52dce729ULL;
    hash ^= 8;
    hash ^= hash >> 33;
    hash *= 0xff51afd7ed558ccdULL;
    hash ^= hash >> 33;
    hash *= 0xc4ceb9fe1a85ec53ULL;
    hash ^= hash >> 33;
    return (int64_t)(hash ^ data);
}

// |v| mod d = Math.abs(v % d) for d < 2^63 (Java's % truncates, so |v % d| = |v| mod d; |INT64_MIN| = 2^63 is exact in u64)
GS_HD uint64_t gs_absmod(int64_t v, uint64_t d, uint64_t magic, int shift) {
    const uint64_t n = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
    if (shift == 0) return 0;  // d == 1
    const uint64_t t = gs_mulhi64(magic, n);
    const uint64_t q = (t + ((n - t) >> 1)) >> (shift - 1);
    return n - q * d;
}
