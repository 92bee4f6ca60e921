// gs_decode.h -- the walk over a handle's store that gs_export.hip (KMerStore.visit) and gs_index.hip (BloomIndexGoal) share:
// four lanes per 64-byte line (record line or table bucket), lane q of the quad holds bytes [16 q, 16 q + 16) from one 16-byte
// load, so that a wave's load instruction covers 16 whole lines.  Record line: lane 0 holds the window planes (w0, w1), lane
// q = 1..3 the value words w(2q), w(2q+1) = offsets j in [6 (q - 1), 6 q) and decodes those from the planes it takes from lane 0.
// Table bucket: lane q decodes slots 2q, 2q + 1.  The layout is reversible: a record line holds its whole window (planes + valid
// bits + value indices), a table slot holds rem | disp | value + 1, and gs_mix_planes is a Feistel bijection (gs_unmix_planes).
// Seen bits (a live unique-counting run) and `more` bits are masked by the field extraction.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_layout.h"

#define GS_EX_MAX_PER_LANE 6  // a lane holds 16 bytes of a line: 6 record offsets or 2 table slots

// the lane's 16 bytes of `line`: record lines [0, n_rec), then table buckets; zero beyond the handle's n_lines
__device__ __forceinline__ void gs_ex_load_quad(const unsigned long long *rec, const unsigned long long *tab, int64_t n_rec, int64_t n_lines,
                                                int64_t line, int q, unsigned long long &x0, unsigned long long &x1) {
    x0 = x1 = 0;
    if (line < n_lines) {
        const uint4 w = line < n_rec ? *reinterpret_cast<const uint4 *>(rec + (size_t)line * GS_REC_WORDS + 2 * q)
                                     : *reinterpret_cast<const uint4 *>(tab + (size_t)(line - n_rec) * GS_SLOTS_PER_BUCKET + 2 * q);
        x0 = ((unsigned long long)w.y << 32) | w.x;
        x1 = ((unsigned long long)w.w << 32) | w.z;
    }
}

// the valid bits of the lane's record offsets 6 (q - 1) + i (w1: the quad's second plane word, valid bits above the window)
__device__ __forceinline__ uint32_t gs_ex_rec_valid(unsigned long long w1, int q) {
    return q > 0 ? (uint32_t)(w1 >> GS_REC_WIN_BITS) >> (6 * (q - 1)) : 0u;
}

// value index of record offset 6 (q - 1) + i in the lane's two value words (three 21-bit fields each, `more` in bit 63)
__device__ __forceinline__ int32_t gs_ex_rec_value(unsigned long long x0, unsigned long long x1, int i) {
    return (int32_t)(((i < 3 ? x0 : x1) >> (GS_REC_VAL_BITS * (i % 3))) & (GS_REC_MAX_VALUES - 1));
}

// value index of a table slot (an empty slot: -1)
__device__ __forceinline__ int32_t gs_ex_tab_value(unsigned long long s, uint32_t vmask) { return (int32_t)((uint32_t)(s >> 1) & vmask) - 1; }

// reference key of record offset j (w0, w1: the quad's plane words)
__device__ __forceinline__ unsigned long long gs_ex_rec_key(unsigned long long w0, unsigned long long w1, int j, int k, uint32_t kmask) {
    const unsigned long long whi = w0 & ((1ULL << GS_REC_WIN_BITS) - 1), wlo = w1 & ((1ULL << GS_REC_WIN_BITS) - 1);
    return gs_planes_to_kmer((uint32_t)(whi >> j) & kmask, (uint32_t)(wlo >> j) & kmask, k);
}

// reference key of table slot s in global bucket `bucket`
__device__ __forceinline__ unsigned long long gs_ex_tab_key(unsigned long long s, unsigned long long bucket, uint32_t vbits, uint32_t bucket_bits, int k,
                                                            uint32_t kmask) {
    const unsigned long long bmask = (1ULL << bucket_bits) - 1;
    const unsigned long long disp = (s >> (vbits + 1)) & 3u, rem = s >> (vbits + 3);
    uint32_t a, b;
    gs_unmix_planes((rem << bucket_bits) | ((bucket - disp) & bmask), a, b);
    return gs_planes_to_kmer(a & kmask, b & kmask, k);
}

// wave prefix of per-lane counts c in 0..7 from three ballots: `before` = the sum over the lower lanes, `total` = over the wave
__device__ __forceinline__ void gs_ex_wave_prefix(int c, int lane, int &before, int &total) {
    const unsigned long long lt = (1ULL << lane) - 1ULL;
    before = total = 0;
    for (int bit = 0; bit < 3; bit++) {
        const unsigned long long m = __ballot((c >> bit) & 1);
        before += __popcll(m & lt) << bit;
        total += __popcll(m) << bit;
    }
}
