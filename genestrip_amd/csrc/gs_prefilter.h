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
