// gs_snrec.h -- every read of the FIXED loop of gs_match_kernel (counters in LDS) leaves the wave as a record, and the kernels of
// gs_snreduce.hip work the records off one lane per record.  What the record of a read of ONE tax id turns into is a pure function
// of (hit0, hit1, vi, read number) and the launch constants: gs_sn_row below, device and host alike (tests/native/snrec_steps.cpp).
// A read of several tax ids or with a non-CGAT byte is its row of node codes: gs_sn_walk (tests/native/snwalk_steps.cpp).
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

// EVERY read of that loop leaves the wave as a record.  Slot t of the array belongs to trip t of the launch: the index into the
// survivor list behind the prefilter, the read's number otherwise.
// vi >= 0: a read without a non-CGAT byte whose hit positions all hold one node.  Every live position of such a read is a hit or a
// MISS, so tax_err = class_err = max - popcount(hits) and the record needs no miss masks.
// vi == GS_SN_NONE: no hit and no non-CGAT byte; (vi, r) alone are written, the reduce kernel writes the read's outputs (-1 / 0).
// vi == GS_SN_NODES: any other read (several nodes, or a non-CGAT byte).  (vi, r, bad) are written, and row t of the batch's node
// codes (GsMatchParams::sn_nodes) holds the node of every position: value index, GS_NODE_MISS, GS_NODE_INVALID or GS_NODE_NONE as
// 16-bit values, position p at [p].  The codes say which WINDOWS hold a non-CGAT byte; how many such BYTES the read has, which is
// what tax_err counts, they do not say (two bytes fewer than k apart and three give the same windows): that count travels in `bad`.
#define GS_SN_NONE (-1)
#define GS_SN_NODES (-2)
#define GS_SN_ROW 128           // codes per row
#define GS_SN_CODE_MAX 0x7fff   // value indices a code can hold
struct GsSnRec {
    uint64_t hit0, hit1;  // hit positions 0 .. 63 and 64 .. 127
    int32_t vi;           // the node, GS_SN_NONE or GS_SN_NODES
    uint32_t r;           // the read's number in the batch
    uint32_t bad;         // GS_SN_NODES: non-CGAT bytes below position max - 1, plus one if there is one at or behind it
    uint32_t unused;      // (32 bytes: a record never straddles two 32-byte sectors)
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

// ---------------------------------------------------------------------------------------------------
// A read that left as its row of node codes (GS_SN_NODES): what gs_process_read does after the probe, restated for ONE lane that
// walks the positions one by one.  Contigs are maximal runs of one value index; the distinct hit nodes are taken in order of first
// appearance (READS_1KMER once each, mergeReadTaxidPath up to max_paths paths); then path sums, ties in path order, the threshold
// mapping, the LCA fold, both gates and quotients from the batch's table.  Counters go to `sink`:
//   sink.add(vi, column of GS_S_*, u64), sink.max_key(vi, key), sink.dadd(vi, column of GS_D_*, double).
// ---------------------------------------------------------------------------------------------------
struct GsSnWalkConst {
    GsSnConst c;
    int32_t max_paths;             // 1 .. 64
    int32_t n_values;
    const int32_t *parent, *tin, *tout;  // the taxonomy (value index == node id; tin/tout: pre-order interval)
};

GS_HD bool gs_sn_anc_or_self(const GsSnWalkConst &w, int a, int x) { return w.tin[a] <= w.tin[x] && w.tin[x] < w.tout[a]; }

GS_HD int gs_sn_lca(const GsSnWalkConst &w, int a, int b) {  // (gs_lca of gs_kernels.hip; -1 == null)
    if (a == b) return a;
    if (a < 0 || b < 0) return -1;
    while (a >= 0 && !gs_sn_anc_or_self(w, a, b)) a = w.parent[a];
    return a;
}

// codes: GS_SN_ROW of them, 16-byte aligned, position p at [p]; only [0, c.max) count.  bad: GsSnRec::bad.
// Two passes.  The first takes the row in as 64 words (wide loads, no index that is not a constant: the words stay in registers) and
// leaves three 128-bit masks -- hit, MISS, "differs from the position in front" -- the second visits the hit contigs alone, a
// handful per read, and reads the node of each from the row again.
template <class Sink>
GS_HD void gs_sn_walk(const uint16_t *codes, uint32_t bad, uint32_t r, int64_t first_read_no, const GsSnWalkConst &w,
                      const GsQuotTable *qt, Sink &sink, int32_t &out_class, int32_t &out_flags) {
    const int max = w.c.max, nv = w.n_values;
    int16_t dvi[GS_SN_ROW];   // distinct hit nodes in order of first appearance
    uint8_t dcnt[GS_SN_ROW];  // positions that hold them, minus one (1 .. 128 positions)
    int16_t path[64];
    int nd = 0;
    out_class = -1;
    out_flags = 0;
    uint32_t word[GS_SN_ROW / 2];
    __builtin_memcpy(word, __builtin_assume_aligned(codes, 16), sizeof(word));
    uint64_t hit[2] = {0, 0}, miss[2] = {0, 0}, chg[2] = {0, 0};
    int prev = -3;  // (GS_NODE_NONE in front of position 0)
#pragma unroll
    for (int p = 0; p < GS_SN_ROW; p++) {
        int v = (int)(int16_t)(uint16_t)(word[p >> 1] >> (16 * (p & 1)));
        if (v >= nv || v < -3) v = -1;  // (no code of the match kernel's: nothing may index with it)
        const uint64_t bit = 1ULL << (p & 63);
        if (v >= 0) hit[p >> 6] |= bit;
        if (v == -1) miss[p >> 6] |= bit;
        if (v != prev) chg[p >> 6] |= bit;
        prev = v;
    }
    const uint64_t live1 = max >= 128 ? ~0ULL : (1ULL << (max - 64)) - 1ULL;  // (64 < max <= 128: word 0 is whole)
    hit[1] &= live1;
    miss[1] &= live1;
    chg[1] &= live1;
    const int n_miss = __builtin_popcountll(miss[0]) + __builtin_popcountll(miss[1]);
    // the hit contigs: a contig starts at a hit position that differs from the one in front and ends in front of the next position
    // that differs, or at max (the tail flush)
    uint64_t s0 = hit[0] & chg[0], s1 = hit[1] & chg[1];
    while ((s0 | s1) != 0) {
        int p;
        if (s0) {
            p = __builtin_ctzll(s0);
            s0 &= s0 - 1;
        } else {
            p = 64 + __builtin_ctzll(s1);
            s1 &= s1 - 1;
        }
        // changes above p
        const uint64_t a0 = p < 63 ? chg[0] & (~0ULL << (p + 1)) : 0ULL;
        const uint64_t a1 = p < 64 ? chg[1] : (p < 127 ? chg[1] & (~0ULL << (p - 63)) : 0ULL);
        const int end = a0 ? __builtin_ctzll(a0) : (a1 ? 64 + __builtin_ctzll(a1) : max);
        const uint32_t len = (uint32_t)(end - p);
        int v = (int)(int16_t)codes[p];
        if (v >= nv || v < 0) continue;  // (cannot be: p is a hit position)
        sink.add(v, GS_S_KMERS, (uint64_t)len);
        sink.add(v, GS_S_CONTIGS, (uint64_t)1);
        sink.add(v, GS_S_CONTIG_LEN_SQ_SUM, (uint64_t)len * len);
        sink.max_key(v, gs_sn_max_key(len, first_read_no, r));
        int dd = 0;
        while (dd < nd && dvi[dd] != v) dd++;
        if (dd == nd) {
            dvi[nd] = (int16_t)v;
            dcnt[nd] = (uint8_t)(len - 1);
            nd++;
        } else
            dcnt[dd] = (uint8_t)(dcnt[dd] + len);
    }
    if (nd == 0) return;  // no hit: nothing is booked, the outputs are -1 / 0
    out_flags = GS_F_FOUND | GS_F_RETURNED;
    int used = 0;
    for (int dd = 0; dd < nd; dd++) {
        const int v = dvi[dd];
        sink.add(v, GS_S_READS_1KMER, (uint64_t)1);  // first k-mer of this tax id in the read
        if (!w.c.classify) continue;
        // mergeReadTaxidPath: the first path (in path order) that is an ancestor or a descendant; a path moves down only
        bool related = false;
        for (int i = 0; i < used && !related; i++) {
            const bool a = gs_sn_anc_or_self(w, path[i], v), b = gs_sn_anc_or_self(w, v, path[i]);
            if (a || b) {
                if (a) path[i] = (int16_t)v;
                related = true;
            }
        }
        if (!related && (used == 0 || used < w.max_paths) && used < 64) path[used++] = (int16_t)v;
    }
    if (!w.c.classify) return;
    int tax_err = n_miss + (int)bad;
    if (tax_err > GS_QUOT_ENTRIES - 1) tax_err = GS_QUOT_ENTRIES - 1;  // (cannot be: tax_err <= max, see GsQuotTable)
    if (((qt->tax_disabled[tax_err >> 5] >> (tax_err & 31)) & 1u) != 0) return;
    // sumCounts per candidate path, max and ties exactly as the in-place scan; tie order = path order
    int best = 0;
    uint64_t ties = 0;
    for (int i = 0; i < used; i++) {
        int sum = 0;
        for (int dd = 0; dd < nd; dd++)
            if (gs_sn_anc_or_self(w, dvi[dd], path[i])) sum += (int)dcnt[dd] + 1;
        if (sum > best) {
            best = sum;
            ties = 0;
        }
        if (sum >= best) ties |= 1ULL << i;
    }
    int cn = -1, first_node = -1;
    bool first = true;
    for (int i = 0; i < used; i++) {
        if (((ties >> i) & 1ULL) == 0) continue;
        int x = path[i];
        if (w.c.threshold > 1) {  // lowestNodeWhereSumAboveThreshold
            int mapped = -1, acc = 0;
            for (int y = path[i]; y >= 0 && mapped < 0; y = w.parent[y])
                for (int dd = 0; dd < nd; dd++)
                    if (dvi[dd] == y) {
                        acc += (int)dcnt[dd] + 1;
                        if (acc >= w.c.threshold) mapped = y;
                    }
            x = mapped;
        }
        if (first) {
            cn = first_node = x;
            first = false;
        } else
            cn = gs_sn_lca(w, cn, x);
    }
    out_class = cn;
    if (cn < 0) {
        out_flags &= ~GS_F_RETURNED;
        return;
    }
    int read_kmers = best;
    if (w.c.threshold > 1) {  // sumCounts(readTaxIdNode[0]) after the promotion
        read_kmers = 0;
        for (int dd = 0; dd < nd; dd++)
            if (gs_sn_anc_or_self(w, dvi[dd], first_node)) read_kmers += (int)dcnt[dd] + 1;
    }
    int class_err = max - read_kmers;
    if (class_err < 0) class_err = 0;  // (cannot be: read_kmers counts positions of this read)
    if (((qt->class_counted[class_err >> 5] >> (class_err & 31)) & 1u) == 0) return;
    out_flags |= GS_F_COUNTED;
    const GsQuotEntry te = qt->e[tax_err], ce = qt->e[class_err];
    sink.add(cn, GS_S_READS, (uint64_t)1);
    sink.add(cn, GS_S_READS_KMERS, (uint64_t)read_kmers);
    sink.add(cn, GS_S_READS_BPS, (uint64_t)w.c.read_len);
    sink.dadd(cn, GS_D_ERR_SUM, te.q);
    sink.dadd(cn, GS_D_ERR_SQ_SUM, te.q2);
    sink.dadd(cn, GS_D_CLASS_ERR_SUM, ce.q);
    sink.dadd(cn, GS_D_CLASS_ERR_SQ_SUM, ce.q2);
}
