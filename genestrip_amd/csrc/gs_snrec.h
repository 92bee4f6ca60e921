// gs_snrec.h -- a read of ONE tax id in the FIXED loop of gs_match_kernel (counters in LDS) leaves the wave as a record, and
// gs_sn_reduce_kernel (gs_snreduce.hip) works the records off one lane per record.  What a record turns into is a pure function of
// (hit0, hit1, vi, read number) and the launch constants: gs_sn_row below, device and host alike (tests/native/snrec_steps.cpp).
// Plain C++ but for GS_HD: no HIP header is needed to include this file.
#pragma once
#include <stdint.h>

#include "../../include/gsgpu.h"
#include "gs_layout.h"

// What a batch of ONE read length (gs_match_submit_fixed, the FIXED loop of gs_match_kernel) knows before its first read: with
// max = read_len - k + 1 <= 128 positions, tax_err and class_err are integers in 0 .. max, so both error gates are one bit per
// value and both quotients one table entry.  Built on the host (launch_batch) with the very expressions of the general loop, in
// plain double arithmetic: i / max is the correctly rounded quotient on the host as on the device.
// (tax_err <= max: a window with a bad base is INVALID, never a MISS, so n_miss + bad_lo counts every position below max - 1 at
// most once, and a bad base behind them (bad_hi) makes the last window INVALID.  class_err = max - read_kmers, 1 <= read_kmers.)
#define GS_QUOT_ENTRIES 129
#define GS_QUOT_WORDS ((GS_QUOT_ENTRIES + 31) / 32)
struct GsQuotEntry {
    double q, q2;  // i / max and its square
};
struct GsQuotTable {
    GsQuotEntry e[GS_QUOT_ENTRIES];
    uint32_t tax_disabled[GS_QUOT_WORDS];   // bit i: tax_err == i fails the max_read_tax_err gate
    uint32_t class_counted[GS_QUOT_WORDS];  // bit i: class_err == i passes the max_read_class_err gate
};

// The record of a read without a non-CGAT byte whose hit positions all hold one node.  Slot t of the array belongs to trip t of the
// launch: the index into the survivor list behind the prefilter, the read's number otherwise.  Every live position of such a read is
// a hit or a MISS, so tax_err = class_err = max - popcount(hits) and the record needs no miss masks.  A read that is not deferred
// writes vi = -1 alone (what lies behind it in the slot is stale).
struct GsSnRec {
    uint64_t hit0, hit1;  // hit positions 0 .. 63 and 64 .. 127
    int32_t vi;           // the node, -1: nothing deferred
    uint32_t r;           // the read's number in the batch
    uint64_t unused;      // (32 bytes: a record never straddles two 32-byte sectors)
};
static_assert(sizeof(GsSnRec) == 32, "GsSnRec");

// the launch constants the reduce needs
struct GsSnConst {
    int32_t max;        // k-mer positions of the batch's one read length, 65 .. 128
    int32_t read_len;
    int32_t classify, threshold;
};

// what a record adds to the tables and what it writes per read
struct GsSnRow {
    uint32_t sums[GS_N_SUMS];  // the read's row of `sums`
    uint32_t longest;          // its longest contig (the max key is (longest << 40) | key_lo)
    int32_t out_class, out_flags;
    int32_t counted, tax_err, class_err;  // counted: the four double columns take e[tax_err] and e[class_err]
};

// a 128-bit mask (lo: bits 0 .. 63) shifted right by n in 0 .. 128
GS_HD void gs_sn_shr(uint64_t &lo, uint64_t &hi, int n) {
    if (n >= 128) {
        lo = hi = 0;
    } else if (n >= 64) {
        lo = hi >> (n - 64);
        hi = 0;
    } else if (n > 0) {
        lo = (lo >> n) | (hi << (64 - n));
        hi >>= n;
    }
}

// (longest << 40) | (2^40 - 1 - (read number mod 2^40)): the key whose maximum is the longest contig of the lowest read number
GS_HD uint64_t gs_sn_max_key(uint32_t longest, int64_t first_read_no, uint32_t r) {
    const uint64_t m40 = (1ULL << 40) - 1;
    return ((uint64_t)longest << 40) | (m40 - ((uint64_t)(first_read_no + (int64_t)r) & m40));
}

// hit0 | hit1 != 0, no bit at or above c.max.  A contig is a maximal run of set bits over the 128 positions (positions >= max hold
// no hit; the run that reaches max - 1 is the tail flush).  The classification is the closed form of a read of one node: the only
// candidate path is vi, its sum and read_kmers are the hit count.
GS_HD void gs_sn_row(uint64_t hit0, uint64_t hit1, int32_t vi, const GsSnConst &c, const GsQuotTable *qt, GsSnRow &o) {
    const int cnt = __builtin_popcountll(hit0) + __builtin_popcountll(hit1);
    uint32_t contigs = 0, sq = 0, longest = 0;
    uint64_t lo = hit0, hi = hit1;
    while ((lo | hi) != 0) {
        gs_sn_shr(lo, hi, lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll(hi));  // to the run's first position
        const uint64_t nlo = ~lo, nhi = ~hi;
        const int l = nlo ? __builtin_ctzll(nlo) : (nhi ? 64 + __builtin_ctzll(nhi) : 128);
        gs_sn_shr(lo, hi, l);
        contigs++;
        sq += (uint32_t)(l * l);  // (at most 128 positions: 128^2 fits)
        longest = (uint32_t)l > longest ? (uint32_t)l : longest;
    }
    o.out_class = -1;
    o.out_flags = GS_F_FOUND | GS_F_RETURNED;
    o.counted = 0;
    o.tax_err = o.class_err = 0;
    if (c.classify) {
        o.tax_err = c.max - cnt;
        if (((qt->tax_disabled[o.tax_err >> 5] >> (o.tax_err & 31)) & 1u) == 0) {
            o.out_class = (c.threshold <= 1 || cnt >= c.threshold) ? vi : -1;
            if (o.out_class < 0) {
                o.out_flags &= ~GS_F_RETURNED;
            } else {
                o.class_err = c.max - cnt;
                o.counted = (int32_t)((qt->class_counted[o.class_err >> 5] >> (o.class_err & 31)) & 1u);
                if (o.counted) o.out_flags |= GS_F_COUNTED;
            }
        }
    }
    o.sums[GS_S_READS] = (uint32_t)o.counted;
    o.sums[GS_S_READS_KMERS] = o.counted ? (uint32_t)cnt : 0u;
    o.sums[GS_S_KMERS] = (uint32_t)cnt;
    o.sums[GS_S_CONTIGS] = contigs;
    o.sums[GS_S_CONTIG_LEN_SQ_SUM] = sq;
    o.sums[GS_S_READS_1KMER] = 1u;
    o.sums[GS_S_READS_BPS] = o.counted ? (uint32_t)c.read_len : 0u;
    o.longest = longest;
}
