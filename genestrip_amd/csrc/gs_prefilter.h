// gs_prefilter.h -- the sampled 15-mer test of a read against a store's 15-mer filter, host and device (gs_prefilter.hip, and
// tests/native/prefilter_emulate.cpp holds these very functions to the Python restatement in tests/prefilter.py).
//
// A stored k-mer at read position s owns the w = k - 14 15-mer positions s .. s + w - 1.  Exactly one of w consecutive positions
// is a multiple of w, and it is <= L - 15 because s <= L - k: the samples are the positions 0, w, 2 w, .. <= L - 15 (eight of them
// at L = 150, k = 31), and every k-mer of the read owns exactly one.
// A read none of whose samples is in S -- the canonical 15-mers (gs_lmer_canon) of every stored k-mer -- holds no stored k-mer.
// Two levels: a one-hash bit table small enough for the L2s, and the exact bit set over the 30-bit canonical code, asked only
// where the first level passed.  A sample that holds a byte which is not C, G, A or T is absent: every window over it is INVALID.
#pragma once
#include <stdint.h>

#include "gs_layout.h"

#define GS_PF_L1_BITS 24                            // first level: 2^24 bits = 2 MiB
#define GS_PF_L2_WORDS ((size_t)1 << (30 - 5))      // exact level: one bit per canonical code, 128 MiB

GS_HD int gs_pf_stride(int k) { return k - (GS_MIN_L - 1); }
GS_HD int gs_pf_samples(int L, int k) { return (L - GS_MIN_L) / gs_pf_stride(k) + 1; }

GS_HD uint32_t gs_pf_l1_bit(uint32_t canon) { return (canon * 0x9E3779B1u) >> (32 - GS_PF_L1_BITS); }

// the four bytes of v, each a base: bit j of the result = code-hi / code-lo bit of byte j (gs_word_from_byte_fixed: hi = bit 1
// clear, lo = bit 2; a byte that is no base gives whatever its bits say -- gs_pf_bad4 tells)
GS_HD uint32_t gs_pf_gather4(uint32_t bits01) { return ((bits01 & 0x01010101u) * 0x01020408u) >> 24; }
GS_HD uint32_t gs_pf_hi4(uint32_t v) { return gs_pf_gather4(~v >> 1) & 15u; }
GS_HD uint32_t gs_pf_lo4(uint32_t v) { return gs_pf_gather4(v >> 2) & 15u; }
// nonzero bytes where v holds a byte that is not one of the upper-case letters C, G, A, T: the letter its bits 1 and 2 select
// (A 0x41, C 0x43, T 0x54, G 0x47) is 0x41 ^ b1 << 1 ^ b2 << 2 ^ 0x11 (b2 & ~b1)
GS_HD uint32_t gs_pf_bad4(uint32_t v) {
    const uint32_t b1 = (v >> 1) & 0x01010101u, b2 = (v >> 2) & 0x01010101u, t = b2 & ~b1;
    return v ^ (0x41414141u ^ (b1 << 1) ^ (b2 << 2) ^ t ^ (t << 4));
}

// the canonical code (30 bits) of the 15 bases in the low 15 bytes of (d0, d1, d2, d3), first base in byte 0 of d0, and whether
// one of the 15 bytes is no base (the code is arbitrary then)
GS_HD uint32_t gs_pf_canon15(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
    const uint32_t fh = gs_pf_hi4(d0) | (gs_pf_hi4(d1) << 4) | (gs_pf_hi4(d2) << 8) | ((gs_pf_hi4(d3) & 7u) << 12);
    const uint32_t fl = gs_pf_lo4(d0) | (gs_pf_lo4(d1) << 4) | (gs_pf_lo4(d2) << 8) | ((gs_pf_lo4(d3) & 7u) << 12);
    return gs_lmer_canon(fh, fl) >> 1;
}
GS_HD uint32_t gs_pf_bad15(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
    return gs_pf_bad4(d0) | gs_pf_bad4(d1) | gs_pf_bad4(d2) | (gs_pf_bad4(d3) & 0x00ffffffu);
}

// the probe: level one, then the exact level, then the bytes (a sample with a byte that is no base has arbitrary planes: it is
// looked at last because it is the rarest way out, and it never lets a read through that the exact test would reject)
GS_HD bool gs_pf_sample_in(const uint32_t *l1, const uint32_t *l2, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
    const uint32_t c = gs_pf_canon15(d0, d1, d2, d3);
    const uint32_t b = gs_pf_l1_bit(c);
    if (((l1[b >> 5] >> (b & 31)) & 1u) == 0) return false;
    if (((l2[c >> 5] >> (c & 31)) & 1u) == 0) return false;
    return gs_pf_bad15(d0, d1, d2, d3) == 0;
}

// gs_pf_canon15 as gs_pf_kernel computes it: the planes gathered by byte dot products (c + the sum of the four byte products of a
// and b, one full-rate instruction on the device) instead of eight quarter-rate 32-bit multiplies.  Equal for every input.
GS_HD uint32_t gs_pf_dot4(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    for (int i = 0; i < 4; i++) c += ((a >> (8 * i)) & 255u) * ((b >> (8 * i)) & 255u);
    return c;
#endif
}
// 2^bit x (bit `bit` of byte j of (d0, d1, d2, d3) in bit j, j < 15); m = that bit in every byte
GS_HD uint32_t gs_pf_plane15(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t m) {
    const uint32_t W0 = 0x08040201u, W1 = 0x80402010u;  // byte j of a dword counts 2^j, of the dword behind it 2^(4 + j)
    return gs_pf_dot4(d0 & m, W0, gs_pf_dot4(d1 & m, W1, 0u)) + (gs_pf_dot4(d2 & m, W0, gs_pf_dot4(d3 & (m & 0x00ffffffu), W1, 0u)) << 8);
}
GS_HD uint32_t gs_pf_canon15_dot(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
    const uint32_t fh = (~gs_pf_plane15(d0, d1, d2, d3, 0x02020202u) >> 1) & 0x7fffu;  // code-hi: bit 1 clear
    const uint32_t fl = gs_pf_plane15(d0, d1, d2, d3, 0x04040404u) >> 2;               // code-lo: bit 2
    return gs_lmer_canon(fh, fl) >> 1;
}

// ---- the test as gs_pf_kernel runs it: the samples of a read in groups of at most GS_PF_GROUP.  The codes of a group are computed
// together and its level-one words loaded together (one latency for the group); then the exact level is asked sample by sample,
// and only for the group's level-one passes, first to last, until one is in S with clean bytes: that sample decides the read.
// The lanes of a wave run the loop in step: every undecided lane asks for the first of its passes it has not asked for yet.
#define GS_PF_GROUP 8
// the groups of a read's m samples: sample 0 alone, then GS_PF_GROUP at a time; s0 = the group's first sample
GS_HD int gs_pf_group_size(int s0, int m) { return s0 == 0 ? 1 : (m - s0 < GS_PF_GROUP ? m - s0 : GS_PF_GROUP); }
// bit i: sample i of the group passed level one (l1w[i] = the level-one word of codes[i])
GS_HD uint32_t gs_pf_group_l1(const uint32_t *codes, const uint32_t *l1w, int n) {
    uint32_t todo = 0;
    for (int i = 0; i < n; i++) todo |= ((l1w[i] >> (gs_pf_l1_bit(codes[i]) & 31)) & 1u) << i;
    return todo;
}
// the exact-level steps of one group: in_s(i) = "sample i of the group is in S and holds bases only" (the exact-level load, then
// the byte check) is asked for the set bits of todo in rising order and never twice.  Returns the deciding sample or -1.
template <class InS>
GS_HD int gs_pf_group_decide(uint32_t todo, InS in_s) {
    while (todo) {
        const int i = __builtin_ctz(todo);
        todo &= todo - 1;
        if (in_s(i)) return i;
    }
    return -1;
}

// ---- the copy of a wave round: nr reads of L bytes that start delta bytes behind a 16-byte boundary of global memory go to the
// wave's buffer in 16-byte pieces, piece c to buffer bytes [16 c, 16 c + 16), so that read r starts at buffer byte delta + r L.
GS_HD int gs_pf_copy_pieces(int delta, int nr, int L) { return (delta + nr * L + 15) >> 4; }
// the buffer bytes [lo, hi) of piece c that lie in the batch: in front of the first read of a batch and behind its last read
// there may be no memory, so the piece at such an end is cut to the reads' own bytes.  Whole (hi - lo = 16): one 16-byte load.
GS_HD void gs_pf_piece_range(int c, int delta, int nr, int L, bool batch_first, bool batch_last, int *lo, int *hi) {
    *lo = 16 * c;
    *hi = 16 * c + 16;
    if (batch_first && *lo < delta) *lo = delta;
    if (batch_last && *hi > delta + nr * L) *hi = delta + nr * L;
}
// bytes of LDS one wave needs for 64 reads of L bytes: the reads, up to 15 bytes in front of them, and the four bytes behind the
// last sample's last dword
GS_HD uint32_t gs_pf_wave_bytes(int L) { return (uint32_t)((64 * L + 15 + 4 + 15) & ~15) + 16u; }

// host form of the whole test (the emulation program and nothing else): bytes of one read -> does it pass?
static inline bool gs_pf_read_passes(const uint32_t *l1, const uint32_t *l2, const uint8_t *rd, int L, int k) {
    const int w = gs_pf_stride(k), m = gs_pf_samples(L, k);
    for (int i = 0; i < m; i++) {
        const uint8_t *p = rd + i * w;
        uint32_t d[4] = {0, 0, 0, 0};
        for (int j = 0; j < GS_MIN_L; j++) d[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
        if (gs_pf_sample_in(l1, l2, d[0], d[1], d[2], d[3])) return true;
    }
    return false;
}
