// gs_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the match hot path.
//
// match: ONE WAVE PER READ.  Lane p owns k-mer start position p; an "iteration" covers 128 positions as two
// sub-rounds of 64, so a 150 bp read at k=31 (120 k-mers) is exactly one iteration.  Per iteration:
//   1. coalesced byte loads of the bases, three 64-lane ballots per 64 bases (code-hi, code-lo, invalid)
//   2. per lane: funnel-shift the ballot planes -> forward k-mer, bit-reverse -> reverse complement,
//      representative orientation (gs_rep_planes), gs_mix_planes -> bucket + remainder
//   3. one 64-byte bucket line per k-mer (4 x dwordx4 per lane, both sub-rounds in flight together)
//   4. per-read reduce inside the wave: contig boundaries by neighbour compare, a wave-uniform loop over
//      the few contig "events" (flush stats / start contig / path merge), unique bitmap by test-then-
//      atomicOr, KrakenUniq-style vote + LCA with O(1) pre-order interval ancestor tests
//   5. per-taxid counters privatised in LDS per workgroup, flushed once with 64-bit global atomics
// The semantics follow C/match/FastqKMerMatcher.java:327-535; the structure does
// not: the reference's rolling/jumping state machine is replaced by its closed form
//   node(p) = INVALID if the window [p,p+k) holds a non-CGAT byte, else store lookup,
//   #INVALID iterations = popcount(bad bases at positions <= max-2) + (any bad base at >= max-1).
// Reads with more than 128 k-mer positions are queued and drained by gs_match_long_kernel, the same code
// iterating with carried state and per-wave scratch counters in HBM instead of in-register lists.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "gs_launch.h"
#include "gs_layout.h"
#include "gs_params.h"
#include "gs_wave.h"

#define GS_LONG_CHUNK 64           // entries of the long-read queue a wave reserves at a time (one atomic per chunk)
#define GS_LONG_NONE 0xffffffffu   // padding of a chunk (a batch holds at most 2^32 - 1 reads)

#if GS_PHASE  // (tools/phase_times.sh; the stamps: gs_wave.h)
extern "C" int gs_debug_phase(unsigned long long *out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(gs_phase_acc), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(gs_phase_acc), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

// ---------------------------------------------------------------------------------------------------
// statistics sinks: LDS-privatised (n_values <= GS_NV_LDS) or direct global atomics
// ---------------------------------------------------------------------------------------------------
// a wave's place in the record array: it takes 64 slots at a time with one atomic and fills them read by read.  The
// cursor lives in LDS (the scalar registers of the read loop are all taken): [0] = base of the chunk, [1] = slots used
// (64: no chunk in hand)
typedef unsigned long long GsRecCursor[2];

struct GsStats {
    u64 *sums;      // [nv][GS_N_SUMS]
    u64 *maxk;      // [nv]
    double *dsums;  // [nv][GS_N_DCOLS]
    // the taxonomy next to the counters: LDS copies when the counters are in LDS (a tree walk is a chain of dependent
    // loads; from HBM/L2 each link costs the better part of a microsecond), the store's arrays otherwise
    const int32_t *parent, *tin, *tout;
    __device__ __forceinline__ void add(int vi, int col, u64 v) const {
        if (!(GS_ABLATE & 8)) atomicAdd(&sums[(size_t)vi * GS_N_SUMS + col], v);
    }
    __device__ __forceinline__ void max(int vi, u64 key) const {
        if (!(GS_ABLATE & 8)) atomicMax(&maxk[vi], key);
    }
    __device__ __forceinline__ void dadd(int vi, int col, double v) const {
        if (!(GS_ABLATE & 8)) atomicAdd(&dsums[(size_t)vi * GS_N_DCOLS + col], v);
    }
    // contig flush (FastqKMerMatcher.java:396-411 / :457-471)
    __device__ __forceinline__ void contig(int vi, int len, u64 key_lo) const {
        add(vi, GS_S_KMERS, (u64)len);
        add(vi, GS_S_CONTIGS, 1);
        add(vi, GS_S_CONTIG_LEN_SQ_SUM, (u64)len * (u64)len);
        max(vi, ((u64)len << 40) | key_lo);
    }
};

// ---------------------------------------------------------------------------------------------------
// tree helpers (value index == node id; tin/tout pre-order interval)
// ---------------------------------------------------------------------------------------------------
// is `a` an ancestor-or-self of `x`  (SmallTaxTree.isAncestorOf(x, a), SmallTaxTree.java:242-252)
__device__ __forceinline__ bool gs_anc_or_self(int a_tin, int a_tout, int x_tin) { return a_tin <= x_tin && x_tin < a_tout; }

template <typename Tree>
__device__ __forceinline__ int gs_lca(const Tree &t, int a, int b) {  // SmallTaxTree.java:263-289, -1 == null
    if (a == b) return a;
    if (a < 0 || b < 0) return -1;
    const int tb = t.tin[b];
    while (a >= 0 && !gs_anc_or_self(t.tin[a], t.tout[a], tb)) a = t.parent[a];
    return a;
}

// per-wave scratch of the long-read kernel, always accessed at agent scope (L1 bypass)
__device__ __forceinline__ int gs_sc_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gs_sc_store(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---------------------------------------------------------------------------------------------------
// one read on one wave.  LONG = false: max <= 128 (one iteration, distinct nodes kept in registers).
// LONG = true: any length; tag/cnt are this wave's scratch rows of n_values ints, serial its read tag.
// WIDE = true: maxClassificationPaths in 65..128 (C/GSConfigKey.java:350 allows 1..128): candidate path i lives in
// lane i & 63 of register set i >> 6; with WIDE = false there is one set and lane = path.
// slot (FIXED): the trip of the launch this read is, its place in P.sn_recs.
// FIXED = true (!LONG): the caller's reads all have ONE length with 65 .. 128 k-mer positions (gs_match_kernel): sub-round 0 is
// full, and the live positions of sub-round 1 come as `live1`, built once per wave; nothing here tests the length.
// ---------------------------------------------------------------------------------------------------
template <bool LONG, bool FROM_NODES, int KC, bool WIDE, bool REC, bool STRIPED, int CTX = 2, bool FIXED = false, bool NOGATE = false>
__device__ __forceinline__ void gs_process_read(const GsMatchParams &P, const GsStats &st, int64_t r, u64 off, int L,
                                                int lane, int (*s_dvi)[128], int (*s_dcnt)[128], int wave_in_block,
                                                int32_t *tag, int32_t *cnt, int serial, const uint32_t (&pre)[3],
                                                uint32_t *wave_g, unsigned long long *cur, u64 live1 = 0, int64_t slot = 0) {
    static_assert(!FIXED || (!LONG && !FROM_NODES), "one iteration, probed here");
    static_assert(!NOGATE || FIXED, "the gate-less probe belongs to the FIXED loop (gs_probe_planes)");
    const GsDbDev &db = P.db;
    const int k = KC ? KC : db.k;
    const int max = L - k + 1;
    const uint8_t *rd = P.seq + off;
    int out_class = -1;
    int out_flags = 0;

    if (FIXED || max > 0) {
        const int64_t read_no = P.first_read_no + r;
        const u64 key_lo = ((1ULL << 40) - 1) - ((u64)read_no & ((1ULL << 40) - 1));
        const int n_iter = LONG ? (max + 127) >> 7 : 1;
        // per-read state
        bool found = false;
        int n_miss = 0, bad_lo = 0;
        bool bad_hi = false;
        int carry_last = GS_NODE_NONE;  // node of the last position of the previous iteration
        int cur_start = 0;
        int dviA = -1, dviB = -1, dcntA = 0, dcntB = 0, nd = 0;  // !LONG: distinct hit nodes (cap 128 >= #contigs)
        int one_vi = -1, one_cnt = 0;                              // !LONG: the first of them, wave-uniform
        bool deferred = false;                                     // REC: its statistics go into a GsStatRec (P.stat_recs)
        int def_contigs = 0, def_max = 0, def_sq = 0;              // (at most 128 positions: 128^2 fits)
        int def_counted = 0, def_read_kmers = 0, def_tax_err = 0;
        // counters in LDS, FIXED loop: no read books anything.  A read with ONE distinct hit node and no non-CGAT byte leaves the
        // wave as a record of its hit masks (GsSnRec, P.sn_recs), a read without a hit as a bare record, any other read as its row
        // of node codes (P.sn_nodes); gs_sn_reduce_kernel and gs_sn_walk_kernel turn them into counters and outputs (gs_snrec.h)
        constexpr bool SN = FIXED && !REC && !WIDE;
        constexpr int NP = WIDE ? 2 : 1;
// "lane 0" on the paths the FIXED loop takes: a literal mask there (a compare's result is kept across the loop in a scalar pair)
#define GS_LANE0 (FIXED ? GS_ACT(1ULL) : lane == 0)
        int path[NP], ptin[NP], ptout[NP], used = 0;            // candidate paths: path i in lane i & 63 of set i >> 6
#pragma unroll
        for (int h = 0; h < NP; h++) {
            path[h] = -1;
            ptin[h] = 0;
            ptout[h] = 0;
        }

        for (int it = 0; it < n_iter; it++) {
            const int base = it << 7;  // first k-mer position of this iteration
            // ---- 1. bases -> ballot planes (3 words cover 128 + k - 1 <= 158 bases)
            u64 Bhi[3], Blo[3], Bbad[3];
#pragma unroll
            for (int w = 0; w < 3; w++) {
                if (LONG)
                    gs_load_word(rd, L, 2 * it + w, lane, Bhi[w], Blo[w], Bbad[w]);
                else if (FIXED)
                    gs_word_from_byte_fixed(pre[w], Bhi[w], Blo[w], Bbad[w]);
                else
                    gs_word_from_byte(pre[w], Bhi[w], Blo[w], Bbad[w]);
            }
            {   // bad-base census for the INVALID-iteration closed form; word 2 belongs to the next iteration
                const int q = max - 1;
                const int nw = (it == n_iter - 1) ? 3 : 2;
#pragma unroll
                for (int w = 0; w < 3; w++) {
                    if (w < nw) {
                        const int lo_bits = q - (base + 64 * w);  // positions of this word that are < q
                        // (FIXED: 64 <= q < 128 -- word 0 whole, of word 1 one position fewer than are live, of word 2 none)
                        const u64 m_lo = FIXED ? (w == 0 ? ~0ULL : (w == 1 ? live1 >> 1 : 0ULL))
                                               : (lo_bits >= 64 ? ~0ULL : (lo_bits <= 0 ? 0ULL : ((1ULL << lo_bits) - 1)));
                        bad_lo += __popcll(Bbad[w] & m_lo);
                        bad_hi = bad_hi || ((Bbad[w] & ~m_lo) != 0);
                    }
                }
            }
            if (!LONG) GS_STAMP(1, (uint32_t)(Bhi[0] ^ Bhi[2]))
            // ---- 2/3. k-mers + probe, both sub-rounds in flight
            int node[2];
            if (FROM_NODES) {
                // DB-partitioned mode: the node of every position was looked up by the owner of its k-mer
                // (gs_probe_keys_kernel on the owning rank) and routed back; INVALID windows carry GS_NODE_INVALID
                const u64 pb = P.pos_off[r] + (u64)base;
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const int p = base + 64 * s + lane;
                    int v = p < max ? P.nodes[pb + 64 * s + lane] : GS_NODE_NONE;
                    // the stream comes from other ranks: a value outside the store's range must not index anything
                    if (p < max && (v >= db.n_values || v < GS_NODE_INVALID)) v = GS_NODE_MISS;
                    node[s] = v;
                }
            } else {
                // (4a. unique k-mers and per-k-mer hit counters are marked by the probe itself)
                const GsMark mk = {P.count_unique, P.hit_counts, STRIPED ? P.bitmap : nullptr,
                                   STRIPED ? P.bitmap + ((db.bucket_mask + 1) * GS_SLOTS_PER_BUCKET >> 5) : nullptr};
#ifndef GS_AGG_ALL
#define GS_AGG_ALL 0
#endif
                const u64 live[2] = {~0ULL, live1};
                gs_probe_planes<KC, STRIPED, CTX, (REC || GS_AGG_ALL) && !LONG, 2, FIXED, NOGATE>(db, Bhi, Blo, Bbad, base, max, lane, node, wave_g, mk, FIXED ? live : nullptr);
            }

            if (!LONG) GS_STAMP(5, node[0] ^ node[1])
            const u64 hit0 = __ballot(node[0] >= 0), hit1 = __ballot(node[1] >= 0);
            found = found || ((hit0 | hit1) != 0);
            n_miss += __popcll(__ballot(node[0] == GS_NODE_MISS)) + __popcll(__ballot(node[1] == GS_NODE_MISS));

            // ---- 4b. contigs and distinct nodes.  Contig statistics are lane parallel: every lane that starts a hit
            // contig finds the next node change in the ballot masks and books the contig itself (:391-413).  Only
            // the DISTINCT hit nodes are walked one by one, in order of first appearance: reads1KMer counts a
            // (read, tax id) pair once (:434-439) and mergeReadTaxidPath (:568-586) is idempotent for a node it
            // has already seen (paths only ever move down the tree), so repeats need no work.  The per-node vote
            // count of the read (incCount, :380-388) is the number of positions holding that node.
            // the first distinct hit node; in ~90 % of the reads that hit a store of species-specific k-mers it is the
            // only one: its id and count stay in scalar registers (one_vi, one_cnt)
            u64 m0 = hit0, m1 = hit1;
#define GS_FIRST_NODE()                                                                                   \
    {                                                                                                     \
        const int j = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1);                                \
        one_vi = j < 64 ? gs_readlane(node[0], j) : gs_readlane(node[1], j - 64);                         \
        const u64 e0 = __ballot(node[0] == one_vi), e1 = __ballot(node[1] == one_vi);                     \
        one_cnt = __popcll(e0) + __popcll(e1);                                                            \
        m0 &= ~e0;                                                                                        \
        m1 &= ~e1;                                                                                        \
        nd = 1;                                                                                           \
    }
            if (REC && (hit0 | hit1) != 0) {  // (needed before the contigs are booked: one record instead of atomics?)
                GS_FIRST_NODE()
                deferred = (m0 | m1) == 0 && P.stat_recs != nullptr;  // one tax id, counters in HBM: no atomics, one record
            }
            if constexpr (SN) {
                // The loop looks k-mers up and nothing else: EVERY read leaves here as a record, and nothing below this block is
                // compiled into the loop (gs_match_kernel enters it only with P.sn_recs and P.sn_nodes in place).
                GsSnRec *const recs = P.sn_recs;
                const bool clean = (Bbad[0] | Bbad[1] | Bbad[2]) == 0;
                int code = GS_SN_NODES;  // several nodes, or a non-CGAT byte: the read is its row of node codes
                if (clean && (hit0 | hit1) == 0) code = GS_SN_NONE;
                if (clean && (hit0 | hit1) != 0) {
                    const int j1 = hit0 ? __builtin_ctzll(hit0) : 64 + __builtin_ctzll(hit1);
                    const int vi1 = j1 < 64 ? gs_readlane(node[0], j1) : gs_readlane(node[1], j1 - 64);
                    if (((hit0 & ~__ballot(node[0] == vi1)) | (hit1 & ~__ballot(node[1] == vi1))) == 0) {
                        // every hit position holds vi1 and no window holds a bad base: the read is its two hit masks.  Lanes
                        // 0 .. 5 take the six words of the record (v_writelane from the scalar values) and store them with one
                        // instruction
                        int w = 0;
                        w = gs_writelane<0>(w, (int)(uint32_t)hit0);
                        w = gs_writelane<1>(w, (int)(uint32_t)(hit0 >> 32));
                        w = gs_writelane<2>(w, (int)(uint32_t)hit1);
                        w = gs_writelane<3>(w, (int)(uint32_t)(hit1 >> 32));
                        w = gs_writelane<4>(w, vi1);
                        w = gs_writelane<5>(w, (int)(uint32_t)r);
                        if (GS_ACT(0x3fULL)) reinterpret_cast<int *>(recs + slot)[lane] = w;
                        GS_STAMP(7, w)
                        return;
                    }
                }
                // (vi, r, bad) by lanes 4 .. 6: the reduce side writes the outputs of a read without a hit and lists a row of codes
                const int bad = bad_lo + (bad_hi ? 1 : 0);
                if (GS_ACT(0x70ULL)) reinterpret_cast<int *>(recs + slot)[lane] = GS_ACT(0x10ULL) ? code : (GS_ACT(0x20ULL) ? (int)(uint32_t)r : bad);
                if (code == GS_SN_NODES) {
                    uint16_t *const row = P.sn_nodes + (size_t)slot * GS_SN_ROW;  // (n_values < 2^15: gs_launch_match)
                    row[lane] = (uint16_t)node[0];
                    row[64 + lane] = (uint16_t)node[1];
                }
                GS_STAMP(7, code)
                return;
            }
            if ((GS_ABLATE & 1) == 0 && ((hit0 | hit1) != 0 || carry_last >= 0)) {
                int prev[2];
                {
                    const int up0 = __shfl_up(node[0], 1);
                    const int up1 = __shfl_up(node[1], 1);
                    const int last0 = gs_readlane(node[0], 63);
                    prev[0] = GS_LANE0 ? carry_last : up0;
                    prev[1] = GS_LANE0 ? last0 : up1;
                }
                // (positions >= max hold NONE: the first of them differs from its predecessor and is masked away; wave-level masks
                // throughout, as in gs_probe_planes)
                const int nv0 = max - base, nv1 = max - base - 64;
                const u64 vm0 = FIXED ? ~0ULL : (nv0 >= 64 ? ~0ULL : (nv0 <= 0 ? 0ULL : ((1ULL << nv0) - 1ULL)));
                const u64 vm1 = FIXED ? live1 : (nv1 >= 64 ? ~0ULL : (nv1 <= 0 ? 0ULL : ((1ULL << nv1) - 1ULL)));
                const u64 chg0 = __ballot(node[0] != prev[0]) & vm0;
                const u64 chg1 = __ballot(node[1] != prev[1]) & vm1;
                // a hit contig left open by the previous iteration ends at the first change of this one
                if (LONG && carry_last >= 0 && (chg0 | chg1) != 0) {
                    const int q = chg0 ? __builtin_ctzll(chg0) : 64 + __builtin_ctzll(chg1);
                    if (lane == 0) st.contig(carry_last, base + q - cur_start, key_lo);
                }
                {   // hit contigs that start here and end before the iteration does
                    const u64 a0 = (chg0 >> 1) >> lane, a1 = (chg1 >> 1) >> lane;  // changes above this lane
                    const int e1 = chg1 ? 64 + __builtin_ctzll(chg1) : -1;
                    const int end0 = a0 ? lane + 1 + __builtin_ctzll(a0) : e1;
                    const int end1 = a1 ? 64 + lane + 1 + __builtin_ctzll(a1) : -1;
                    // a lane books a contig if it starts a hit contig (hit and change) and a later change closes it: in word 0
                    // any change of word 1 or a change above the lane, in word 1 a change above the lane
                    const u64 c0m = hit0 & chg0 & (chg1 ? ~0ULL : (chg0 ? (1ULL << (63 - __builtin_clzll(chg0))) - 1ULL : 0ULL));
                    const u64 c1m = hit1 & chg1 & (chg1 ? (1ULL << (63 - __builtin_clzll(chg1))) - 1ULL : 0ULL);
                    const bool c0 = GS_ACT(c0m), c1 = GS_ACT(c1m);
                    if (REC && deferred) {  // every contig belongs to one_vi: add them up in scalar registers
                        const int len0 = c0 ? end0 - lane : 0, len1 = c1 ? end1 - 64 - lane : 0;
                        for (u64 sm = c0m; sm; sm &= sm - 1) {
                            const int l = gs_readlane(len0, __builtin_ctzll(sm));
                            def_contigs++;
                            def_sq += l * l;
                            def_max = l > def_max ? l : def_max;
                        }
                        for (u64 sm = c1m; sm; sm &= sm - 1) {
                            const int l = gs_readlane(len1, __builtin_ctzll(sm));
                            def_contigs++;
                            def_sq += l * l;
                            def_max = l > def_max ? l : def_max;
                        }
                    } else {
                        if (c0) st.contig(node[0], end0 - lane, key_lo);
                        if (c1) st.contig(node[1], end1 - 64 - lane, key_lo);
                    }
                }
                // start of the contig that is still open at the end of this iteration
                if (chg1)
                    cur_start = base + 127 - __builtin_clzll(chg1);
                else if (chg0)
                    cur_start = base + 63 - __builtin_clzll(chg0);
                // distinct hit nodes of this iteration, in order of first appearance (the first one is known already;
                // the candidate-path state is set up only if a second node follows)
                if (!LONG) {
                    if (!REC) GS_FIRST_NODE()
                    if (!(REC && deferred) && GS_LANE0) st.add(one_vi, GS_S_READS_1KMER, 1);  // first k-mer of this tax id in the read (:434-439)
                    if ((m0 | m1) != 0) {
                        if (GS_LANE0) {
                            dviA = one_vi;
                            dcntA = one_cnt;
                        }
                        if (P.classify) {  // mergeReadTaxidPath into the empty list (max_paths >= 1)
                            if (GS_LANE0) {
                                path[0] = one_vi;
                                ptin[0] = st.tin[one_vi];
                                ptout[0] = st.tout[one_vi];
                            }
                            used = 1;
                        }
                    }
                }
                while ((m0 | m1) != 0) {
                    const int j = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1);
                    const int nvj = j < 64 ? gs_readlane(node[0], j) : gs_readlane(node[1], j - 64);
                    const u64 e0 = __ballot(node[0] == nvj), e1 = __ballot(node[1] == nvj);
                    const int c = __popcll(e0) + __popcll(e1);
                    m0 &= ~e0;
                    m1 &= ~e1;
                    bool first = true;
                    if (LONG) {
                        int f = 0;
                        if (lane == 0) {
                            f = gs_sc_load(tag + nvj) != serial;
                            if (f) gs_sc_store(tag + nvj, serial);
                            gs_sc_store(cnt + nvj, f ? c : gs_sc_load(cnt + nvj) + c);
                        }
                        first = gs_rfl(f) != 0;
                    } else {  // one iteration per read: every node of the walk is new
                        if (nd < 64) {
                            if (lane == nd) {
                                dviA = nvj;
                                dcntA = c;
                            }
                        } else if (lane == nd - 64) {
                            dviB = nvj;
                            dcntB = c;
                        }
                        nd++;
                    }
                    if (first) {
                        // first k-mer of this tax id in the read (:434-439)
                        if (GS_LANE0) st.add(nvj, GS_S_READS_1KMER, 1);
                        if (P.classify) {  // mergeReadTaxidPath (:568-586)
                            const int ntin = st.tin[nvj], ntout = st.tout[nvj];
                            bool related = false;  // the first path (in path order) that is an ancestor or a descendant
#pragma unroll
                            for (int h = 0; h < NP; h++) {
                                if (!related) {
                                    const bool mine = 64 * h + lane < used;
                                    const bool a = mine && gs_anc_or_self(ptin[h], ptout[h], ntin);  // path anc-or-self of node
                                    const bool b = mine && gs_anc_or_self(ntin, ntout, ptin[h]);     // node anc-or-self of path
                                    const u64 m = __ballot(a || b);
                                    if (m) {
                                        const int i = __builtin_ctzll(m);
                                        if (lane == i && a) {
                                            path[h] = nvj;
                                            ptin[h] = ntin;
                                            ptout[h] = ntout;
                                        }
                                        related = true;
                                    }
                                }
                            }
                            if (!related && used < P.max_paths) {
#pragma unroll
                                for (int h = 0; h < NP; h++) {
                                    if (64 * h + lane == used) {
                                        path[h] = nvj;
                                        ptin[h] = ntin;
                                        ptout[h] = ntout;
                                    }
                                }
                                used++;
                            }
                        }
                    }
                }
            }
            if (!LONG) GS_STAMP(6, node[0])
            {   // carry: node of the last valid position of this iteration
                const int last_p = (max - 1 < base + 127) ? max - 1 : base + 127;
                const int ls = FIXED ? 1 : (last_p - base) >> 6, ll = FIXED ? max - 65 : (last_p - base) & 63;  // (FIXED: 64 < max <= 128)
                carry_last = gs_readlane(ls ? node[1] : node[0], ll);
            }
        }

        if ((GS_ABLATE & 1) == 0 && found) {
            out_flags = GS_F_FOUND | GS_F_RETURNED;
            // tail flush (:455-473): the last contig if it is a hit contig
            if (carry_last >= 0) {
                const int len = max - cur_start;
                if (REC && deferred) {
                    def_contigs++;
                    def_sq += len * len;
                    def_max = len > def_max ? len : def_max;
                } else if (GS_LANE0)
                    st.contig(carry_last, len, key_lo);
            }
            // ---- 4c. classification (:474-531)
            if (P.classify) {
                const int tax_err = n_miss + bad_lo + (bad_hi ? 1 : 0);
                // FIXED: max is the batch's, so both gates are one bit per error count and both quotients one entry of the batch's table
                // (GsQuotTable, built by launch_batch from the expressions below); the counts are wave-uniform, the table is read
                // through the scalar cache and no double arithmetic is left in this loop
                typedef const __attribute__((address_space(4))) GsQuotTable *GsQuotPtr;
                const GsQuotPtr qt = FIXED ? (GsQuotPtr)P.quot : nullptr;
                bool disabled;
                if (FIXED) {
                    disabled = ((qt->tax_disabled[tax_err >> 5] >> (tax_err & 31)) & 1u) != 0;
                } else {
                    const double m = P.max_read_tax_err;
                    disabled = m >= 0 && ((m >= 1 && (double)tax_err > m) || ((double)tax_err > m * (double)max));
                }
                if (!disabled) {
                    int cn = -1, first_node = -1, best = 0;
                    // one distinct node v with c positions: the only candidate path is v, its sum is c, and the threshold
                    // mapping (:488-492) keeps v if c >= threshold and finds nothing above it otherwise
                    const bool single = !LONG && nd == 1;
                    if (single) {
                        best = one_cnt;
                        cn = (P.threshold <= 1 || one_cnt >= P.threshold) ? one_vi : -1;
                    } else {
                    // sumCounts per candidate path (SmallTaxTree.java:184-193): lanes = paths
                    int sum[NP];
#pragma unroll
                    for (int h = 0; h < NP; h++) sum[h] = 0;
                    if (LONG) {
#pragma unroll
                        for (int h = 0; h < NP; h++)
                            if (64 * h + lane < used)
                                for (int x = path[h]; x >= 0; x = st.parent[x])
                                    if (gs_sc_load(tag + x) == serial) sum[h] += gs_sc_load(cnt + x);
                    } else {
                        for (int dd = 0; dd < nd; dd++) {
                            const int v = dd < 64 ? gs_readlane(dviA, dd) : gs_readlane(dviB, dd - 64);
                            const int c = dd < 64 ? gs_readlane(dcntA, dd) : gs_readlane(dcntB, dd - 64);
#pragma unroll
                            for (int h = 0; h < NP; h++)
                                if (64 * h + lane < used && gs_anc_or_self(st.tin[v], st.tout[v], ptin[h])) sum[h] += c;
                        }
                    }
                    // max + ties exactly as the in-place scan (:476-487); tie order = path order
                    u64 tie_mask[NP];
#pragma unroll
                    for (int h = 0; h < NP; h++) tie_mask[h] = 0;
                    for (int i = 0; i < used; i++) {
                        const int si = (!WIDE || i < 64) ? gs_readlane(sum[0], i) : gs_readlane(sum[NP - 1], i - 64);
                        if (si > best) {
                            best = si;
#pragma unroll
                            for (int h = 0; h < NP; h++) tie_mask[h] = 0;
                        }
                        if (si >= best) {
                            if (!WIDE || i < 64)
                                tie_mask[0] |= 1ULL << i;
                            else
                                tie_mask[NP - 1] |= 1ULL << (i - 64);
                        }
                    }
                    int cand[NP];  // per tied lane: the node entering the LCA fold
#pragma unroll
                    for (int h = 0; h < NP; h++) cand[h] = path[h];
                    if (P.threshold > 1) {
                        // lowestNodeWhereSumAboveThreshold per tied path (SmallTaxTree.java:208-221)
                        if (!LONG) {
                            s_dvi[wave_in_block][lane] = dviA;
                            s_dcnt[wave_in_block][lane] = dcntA;
                            s_dvi[wave_in_block][64 + lane] = dviB;
                            s_dcnt[wave_in_block][64 + lane] = dcntB;
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        }
#pragma unroll
                        for (int h = 0; h < NP; h++) {
                            int mapped = -1;
                            if ((tie_mask[h] >> lane) & 1ULL) {
                                int acc = 0;
                                for (int x = path[h]; x >= 0 && mapped < 0; x = st.parent[x]) {
                                    if (LONG) {
                                        if (gs_sc_load(tag + x) == serial) {
                                            acc += gs_sc_load(cnt + x);
                                            if (acc >= P.threshold) mapped = x;
                                        }
                                    } else {
                                        for (int dd = 0; dd < nd; dd++)
                                            if (s_dvi[wave_in_block][dd] == x) {
                                                acc += s_dcnt[wave_in_block][dd];
                                                if (acc >= P.threshold) mapped = x;
                                            }
                                    }
                                }
                            }
                            cand[h] = mapped;
                        }
                    }
                    {
                        bool first = true;
#pragma unroll
                        for (int h = 0; h < NP; h++) {
                            u64 tm = tie_mask[h];
                            while (tm) {
                                const int i = __builtin_ctzll(tm);
                                tm &= tm - 1;
                                const int x = gs_readlane(cand[h], i);
                                if (first) {
                                    cn = x;
                                    first_node = x;
                                    first = false;
                                } else
                                    cn = gs_lca(st, cn, x);
                            }
                        }
                    }
                    }  // !single
                    out_class = cn;
                    if (cn < 0) {
                        out_flags &= ~GS_F_RETURNED;  // "return false" (:497-500)
                    } else {
                        int read_kmers = best;
                        if (P.threshold > 1 && !single) {  // sumCounts(readTaxIdNode[0]) after the promotion (:506-507)
                            read_kmers = 0;
                            if (LONG) {
                                for (int x = first_node; x >= 0; x = st.parent[x])
                                    if (gs_sc_load(tag + x) == serial) read_kmers += gs_sc_load(cnt + x);
                            } else {
                                const int ft = st.tin[first_node];
                                for (int dd = 0; dd < nd; dd++) {
                                    const int v = dd < 64 ? gs_readlane(dviA, dd) : gs_readlane(dviB, dd - 64);
                                    const int c = dd < 64 ? gs_readlane(dcntA, dd) : gs_readlane(dcntB, dd - 64);
                                    if (gs_anc_or_self(st.tin[v], st.tout[v], ft)) read_kmers += c;
                                }
                            }
                        }
                        const int class_err = FIXED ? gs_rfl(max - read_kmers) : max - read_kmers;
                        bool counted;
                        if (FIXED) {
                            counted = ((qt->class_counted[class_err >> 5] >> (class_err & 31)) & 1u) != 0;
                        } else {
                            const double mc = P.max_read_class_err;
                            counted = mc < 0 || (mc >= 1 && (double)class_err <= mc) || ((double)class_err <= mc * (double)max);
                        }
                        if (counted) {
                            out_flags |= GS_F_COUNTED;
                            if (REC && deferred) {  // (cn == one_vi: the only candidate)
                                def_counted = 1;
                                def_read_kmers = read_kmers;
                                def_tax_err = tax_err;
                            } else if (FIXED) {
                                const double err = qt->e[tax_err].q, err_sq = qt->e[tax_err].q2;  // (16 bytes each: one scalar load)
                                const double cerr = qt->e[class_err].q, cerr_sq = qt->e[class_err].q2;
                                if (GS_LANE0) {
                                    st.add(cn, GS_S_READS, 1);
                                    st.add(cn, GS_S_READS_KMERS, (u64)read_kmers);
                                    st.add(cn, GS_S_READS_BPS, (u64)L);
                                    st.dadd(cn, GS_D_ERR_SUM, err);
                                    st.dadd(cn, GS_D_ERR_SQ_SUM, err_sq);
                                    st.dadd(cn, GS_D_CLASS_ERR_SUM, cerr);
                                    st.dadd(cn, GS_D_CLASS_ERR_SQ_SUM, cerr_sq);
                                }
                            } else if (lane == 0) {
                                const double err = (double)tax_err / (double)max;
                                const double cerr = (double)class_err / (double)max;
                                st.add(cn, GS_S_READS, 1);
                                st.add(cn, GS_S_READS_KMERS, (u64)read_kmers);
                                st.add(cn, GS_S_READS_BPS, (u64)L);
                                st.dadd(cn, GS_D_ERR_SUM, err);
                                st.dadd(cn, GS_D_ERR_SQ_SUM, err * err);
                                st.dadd(cn, GS_D_CLASS_ERR_SUM, cerr);
                                st.dadd(cn, GS_D_CLASS_ERR_SQ_SUM, cerr * cerr);
                            }
                        }
                    }
                }
            }
        }
        if (REC && deferred && lane == 0) {
            u64 rbase = cur[0], used = cur[1];
            if (used == 64) {  // a fresh chunk of 64 records for this wave
                rbase = atomicAdd(P.stat_rec_count, 64ULL);
                used = 0;
                cur[0] = rbase;
            }
            cur[1] = used + 1;
            GsStatRec rec;
            rec.vi = one_vi;
            rec.contigs = def_contigs;
            rec.kmers = one_cnt;
            rec.sq = def_sq;
            rec.max_key = ((u64)def_max << 40) | key_lo;
            rec.counted = def_counted;
            rec.read_kmers = def_read_kmers;
            rec.read_len = L;
            rec.n_pos = max;
            rec.tax_err = def_tax_err;
            rec.pad[0] = rec.pad[1] = rec.pad[2] = 0;
            P.stat_recs[rbase + used] = rec;
        }
    }
    if (FIXED) {
        // one wave-uniform test for "no per-read output at all" (a resident batch that only wants the tables) in front of the lane-0
        // region, both pointers fetched together, lane 0 as a literal mask
        int32_t *const cv = P.class_vi;
        uint8_t *const fl = P.flags;
        if (((uintptr_t)cv | (uintptr_t)fl) != 0 && GS_ACT(1ULL)) {
            if (cv) cv[r] = out_class;
            if (fl) fl[r] = (uint8_t)out_flags;
        }
    } else if (lane == 0) {
        if (P.class_vi) P.class_vi[r] = out_class;
        if (P.flags) P.flags[r] = (uint8_t)out_flags;
    }
    if (!LONG) GS_STAMP(7, out_class)
}
#undef GS_LANE0

// ---------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------
// dynamic LDS: [nv*GS_N_SUMS u64 sums][nv u64 max keys][nv*GS_N_DCOLS doubles][3*nv int32 tree] -- sized to the store's value count
// so that small taxonomies do not cap the occupancy
#define GS_STATS_PROLOGUE()                                                                           \
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_dyn_lds[];                        \
    const int nv = P.db.n_values;                                                                     \
    u64 *s_sums = reinterpret_cast<u64 *>(gs_dyn_lds);                                                \
    u64 *s_max = s_sums + (LDS_STATS ? nv * GS_N_SUMS : 0);                                           \
    double *s_d = reinterpret_cast<double *>(s_max + (LDS_STATS ? nv : 0));                           \
    int32_t *s_tree = reinterpret_cast<int32_t *>(s_d + (LDS_STATS ? nv * GS_N_DCOLS : 0));           \
    if (LDS_STATS) {                                                                                  \
        for (int i = threadIdx.x; i < nv * GS_N_SUMS; i += blockDim.x) s_sums[i] = 0;                 \
        for (int i = threadIdx.x; i < nv; i += blockDim.x) s_max[i] = 0;                              \
        for (int i = threadIdx.x; i < nv * GS_N_DCOLS; i += blockDim.x) s_d[i] = 0.0;                 \
        for (int i = threadIdx.x; i < nv; i += blockDim.x) {                                          \
            s_tree[i] = P.db.parent[i];                                                               \
            s_tree[nv + i] = P.db.tin[i];                                                             \
            s_tree[2 * nv + i] = P.db.tout[i];                                                        \
        }                                                                                             \
        __syncthreads();                                                                              \
    }                                                                                                 \
    const bool tree_lds = !LDS_STATS && nv <= GS_NV_TREE_LDS; /* counters too big for LDS, the tree is not */ \
    if (tree_lds) {                                                                                   \
        for (int i = threadIdx.x; i < nv; i += blockDim.x) {                                          \
            s_tree[i] = P.db.parent[i];                                                               \
            s_tree[nv + i] = P.db.tin[i];                                                             \
            s_tree[2 * nv + i] = P.db.tout[i];                                                        \
        }                                                                                             \
        __syncthreads();                                                                              \
    }                                                                                                 \
    GsStats st;                                                                                       \
    if (LDS_STATS) {                                                                                  \
        st.sums = s_sums;                                                                             \
        st.maxk = s_max;                                                                              \
        st.dsums = s_d;                                                                               \
        st.parent = s_tree;                                                                           \
        st.tin = s_tree + nv;                                                                         \
        st.tout = s_tree + 2 * nv;                                                                    \
    } else {                                                                                          \
        const size_t copy = P.stat_copies > 1 ? (size_t)(blockIdx.x % (unsigned)P.stat_copies) : 0;   \
        st.sums = (u64 *)P.sums + copy * (size_t)nv * GS_N_SUMS;                                      \
        st.maxk = (u64 *)P.max_keys + copy * (size_t)nv;                                              \
        st.dsums = P.dsums + copy * (size_t)nv * GS_N_DCOLS;                                          \
        st.parent = tree_lds ? s_tree : P.db.parent;                                                  \
        st.tin = tree_lds ? s_tree + nv : P.db.tin;                                                   \
        st.tout = tree_lds ? s_tree + 2 * nv : P.db.tout;                                             \
    }

#define GS_STATS_EPILOGUE()                                                                           \
    if (LDS_STATS) {                                                                                  \
        __syncthreads();                                                                              \
        const size_t ecopy = P.stat_copies > 1 ? (size_t)(blockIdx.x % (unsigned)P.stat_copies) : 0;  \
        for (int i = threadIdx.x; i < nv * GS_N_SUMS; i += blockDim.x)                                \
            if (s_sums[i]) atomicAdd((u64 *)P.sums + ecopy * (size_t)nv * GS_N_SUMS + i, s_sums[i]);  \
        for (int i = threadIdx.x; i < nv; i += blockDim.x)                                            \
            if (s_max[i]) atomicMax((u64 *)P.max_keys + ecopy * (size_t)nv + i, s_max[i]);            \
        for (int i = threadIdx.x; i < nv * GS_N_DCOLS; i += blockDim.x)                               \
            if (s_d[i] != 0.0) atomicAdd(P.dsums + ecopy * (size_t)nv * GS_N_DCOLS + i, s_d[i]);      \
    }

// ---------------------------------------------------------------------------------------------------
// Which kernel takes which read of a batch with an offsets array: up to 128 k-mer positions gs_match_kernel (which skips the others);
// 129 .. 192 / 193 .. 256 positions gs_match_wide_kernel<3 / 4> where wide_mask says it serves this run (queues 1 / 2); more
// gs_match_long_kernel (queue 0); huge_min positions and more the kernels that cut a read into chunks over many waves (the first
// huge_slots of a batch).  A queue is a dense list of read numbers.  One thread per read and round, GS_CLS_READS reads per workgroup:
// first the workgroup counts its reads per class (in LDS), ONE atomic per class reserves their places, then every read is written to
// its place.  (Queued by gs_match_kernel itself -- one atomic per 64 reads and wave, all on one address -- 9.4 M reads of 159 bp cost
// 1.9 ms: atomics on one address execute one after the other, about 11 ns each.)
// ---------------------------------------------------------------------------------------------------
#define GS_CLS_THREADS 1024
#define GS_CLS_ROUNDS 8
#define GS_CLS_READS (GS_CLS_THREADS * GS_CLS_ROUNDS)
__global__ __launch_bounds__(GS_CLS_THREADS) void gs_classify_kernel(GsMatchParams P, int from_nodes) {
    __shared__ unsigned int s_n[4], s_base[4];
    if (P.skip != nullptr && *P.skip != 0) return;
    if (threadIdx.x < 4) s_n[threadIdx.x] = 0;
    __syncthreads();
    const int lane = gs_lane();
    const int k = P.db.k;
    const int64_t b0 = (int64_t)blockIdx.x * GS_CLS_READS;
    unsigned int place[GS_CLS_ROUNDS];  // class << 30 | place among the workgroup's reads of that class
#pragma unroll
    for (int j = 0; j < GS_CLS_ROUNDS; j++) {
        const int64_t r = b0 + (int64_t)j * GS_CLS_THREADS + threadIdx.x;
        int cls = 0;  // 0: gs_match_kernel; 1 / 2: wide queues; 3: long-read queue (queue 0); huge reads take a slot or class 3
        if (r < P.n_reads) {
            int L;
            if (P.off_stride == 0)
                L = P.fixed_len;
            else {
                const uint64_t *po = P.off + r * P.off_stride;
                L = (int)(po[1] - po[0]);
            }
            const int pos = L - k + 1;
            if (pos > 128) {
                cls = (pos <= 192 && (P.wide_mask & 1)) ? 1 : ((pos <= 256 && (P.wide_mask & 2)) ? 2 : 3);
                if (!from_nodes && P.huge_count != nullptr && pos >= P.huge_min) {
                    const unsigned int slot = atomicAdd(P.huge_count, 1u);  // (rare: contigs, chromosomes)
                    if (slot < (unsigned int)P.huge_slots) {
                        P.huge_list[slot] = (uint32_t)r;
                        cls = 0;
                    } else
                        cls = 3;
                }
            }
        }
        unsigned int pl = 0;
#pragma unroll
        for (int c = 1; c <= 3; c++) {
            const u64 m = __ballot(cls == c);
            if (m != 0) {  // (wave-uniform)
                unsigned int wb = 0;
                if (lane == 0) wb = atomicAdd(&s_n[c], (unsigned int)__popcll(m));
                wb = (unsigned int)gs_rfl((int)wb);
                if (cls == c) pl = ((unsigned int)c << 30) | (wb + (unsigned int)__popcll(m & ((1ULL << lane) - 1ULL)));
            }
        }
        place[j] = pl;
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x <= 3 && s_n[threadIdx.x] != 0) s_base[threadIdx.x] = atomicAdd(P.long_count + 2 * (threadIdx.x % 3), s_n[threadIdx.x]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < GS_CLS_ROUNDS; j++) {
        const unsigned int c = place[j] >> 30;
        if (c != 0) P.long_list[(size_t)(c % 3) * (size_t)P.long_cap + s_base[c] + (place[j] & 0x3fffffffu)] = (uint32_t)(b0 + (int64_t)j * GS_CLS_THREADS + threadIdx.x);
    }
}
extern "C" hipError_t gs_launch_classify(const GsMatchParams *P, hipStream_t stream) {
    if (P->n_reads <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_classify_kernel, dim3((unsigned)((P->n_reads + GS_CLS_READS - 1) / GS_CLS_READS)), dim3(GS_CLS_THREADS), 0, stream, *P, P->nodes != nullptr ? 1 : 0);
    return hipGetLastError();
}

template <bool LDS_STATS, bool FROM_NODES, int KC, bool WIDE = false, bool STRIPED = false, int CTX = 0>
__global__ __launch_bounds__(GS_BLOCK) __attribute__((amdgpu_waves_per_eu(GS_WAVES, GS_WAVES))) void gs_match_kernel(GsMatchParams P) {
    GS_STATS_PROLOGUE()
    __shared__ int s_dvi[GS_BLOCK / 64][128];  // distinct-node list copy, threshold > 1 only
    __shared__ int s_dcnt[GS_BLOCK / 64][128];
    // 15-mer order hashes of the wave's current 144 positions (+ the stripe pointers)
    __shared__ __attribute__((aligned(8))) uint32_t s_g[GS_BLOCK / 64][2 * GS_ROW + (STRIPED ? GS_STRIPE_WORDS : 0)];
    const int lane = gs_lane();
    const int wave_in_block = gs_rfl((int)(threadIdx.x >> 6));  // wave-uniform: per-read bookkeeping runs on the scalar unit
    const int64_t wave_id = (int64_t)blockIdx.x * (GS_BLOCK / 64) + wave_in_block;
    const int64_t n_waves = (int64_t)gs_rfl((int)gridDim.x) * (GS_BLOCK / 64);
    const int k = KC ? KC : P.db.k;
    // The ~40 launch parameters do not fit the scalar register file next to the ballot planes; kept live across
    // the loop they are spilled to VGPR lanes and read back with v_readlane on every use.  Re-reading them from
    // the kernarg segment (scalar cache) once per read is cheaper: the empty asm hides from the compiler that the
    // pointer is loop invariant, so the s_loads stay inside the loop.
    typedef const __attribute__((address_space(4))) GsMatchParams *GsKernargPtr;
    const GsKernargPtr kp0 = (GsKernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    // text mode: a chunk that the device-side record scan refused is skipped as a whole (gs_text.hip)
    const int64_t n_reads = (P.skip != nullptr && *P.skip != 0) ? 0 : P.n_reads;
    __shared__ GsRecCursor s_cur[GS_BLOCK / 64];
    if (lane == 0) {
        s_cur[wave_in_block][0] = 0;
        s_cur[wave_in_block][1] = 64;
    }
    GS_STRIPE_TABLE((const GsMatchParams *)kp0)
#if GS_PHASE
    if (lane < 16) gs_phase_row()[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    gs_stamp(-1);
#endif
    // (Software pipelines over the wave's reads were measured again in round 3, after the LDS and gate round trips had been batched:
    // (1) the bases of the next read into a second LDS buffer by LDS-DMA and the offsets two reads ahead, requested at the top of
    // the iteration: 7.59 -> 7.77 ms on configs[1] -- requests OLDER than the gate loads are waited for with them (in-order
    // counter), the latency only moves; (2) the same requests issued behind the gate loads, the youngest at every later wait: the
    // waits for offsets and bases shrink from 3 250 to 1 650 wave cycles per read (tools/phase_times.sh) and every other phase
    // grows by as much: 7.62 ms, 47 M-k-mer store 9.22 -> 9.41 ms.  The SIMD is short of issue slots, not of overlap.)
    // A batch of ONE read length (gs_match_submit_fixed) pays for its length once: what the length alone decides -- which lanes of the
    // third base word hold a base, which positions of sub-round 1 hold a k-mer, that words 0 and 1 and sub-round 0 are full, that
    // the read is this kernel's at all -- is settled here, per wave, and the loop over the reads tests no length.  For lengths of
    // 128 .. k + 127 bases (65 .. 128 positions at k <= 64); any other length, and any batch with offsets, takes the general loop.
    // The empty asm below hides that fixed_len is loop invariant, so the compiler cannot do this itself.  Both loops are one body
    // of code (`fixed` is a type: std::true_type / std::false_type), and they live in one kernel: an instantiation per
    // (LDS_STATS, KC, CTX) is what the launchers, the occupancy query and the profiles' kernel names know.
    constexpr bool CAN_FIX = !FROM_NODES && !WIDE && !STRIPED;
    const int fixed_L = P.fixed_len;
    // (launch_batch hands a GsQuotTable to exactly these batches; the FIXED loop reads its gates and quotients from it)
    // (counters in LDS: that loop only looks k-mers up and every read leaves it as a record, so it needs room for the records and
    // the rows of node codes; a batch without them -- GS_SN_DEFER=0 -- takes the general loop)
    const bool fixed_batch = CAN_FIX && P.off_stride == 0 && fixed_L >= 128 && fixed_L - k + 1 <= 128 && P.quot != nullptr &&
                             (!LDS_STATS || (P.sn_recs != nullptr && P.sn_nodes != nullptr));
    const u64 fixed_live1 = gs_low_mask(fixed_L - k + 1 - 64);
    // A third variant of the loop: the FIXED loop whose probe leaves the minimizer gate out (gs_probe_planes<.., NOGATE>), for the
    // batches launch_batch marks with P.fixed_nogate -- reads that passed the prefilter, for which the gate says "pass" in nearly
    // every lane.  Only on a store that has both a gate and records (without records the gate saves a bucket line per k-mer), and
    // only where the gate word's hint bits are not used (CTX == 0, one store).
    constexpr bool CAN_NOGATE = CAN_FIX && CTX == 0;
    const bool nogate_batch = CAN_NOGATE && fixed_batch && P.fixed_nogate != 0 && P.db.mgate != nullptr && P.db.rec != nullptr;
    auto reads = [&](auto fixed, auto nogate) {
        constexpr bool FIXED = decltype(fixed)::value;
        constexpr bool NOGATE = decltype(nogate)::value;
        const int64_t po_step = n_waves * P.off_stride;        // stride 1: running offsets; 2: (start, end) pairs
        const uint64_t *po = P.off + wave_id * P.off_stride;   // offsets of the current read
        // FIXED: the wave's trips are counted down on the scalar unit (gfx9 has no scalar 64-bit ordered compare: `r < n_reads` is two
        // spill-lane reads, a vector compare and a branch on vcc per read).  A batch holds fewer than 2^32 reads (launch_batch)
        uint32_t trips = 0;
        // Behind the prefilter (gs_prefilter.hip) the launch takes the reads of a list: trip i reads surv_list[i], and the list's length
        // is in device memory as *P.skip is.  Wave-uniform like fixed_batch, from the kernel's arguments: scalar loads, no other kernel.
        typedef const __attribute__((address_space(4))) uint32_t *GsSurvPtr;
        int64_t n_trips = n_reads;
        // (a batch of one length that takes the general loop -- off_stride 0 -- takes the list too)
        if (P.surv_list != nullptr) n_trips = (int64_t)*(GsSurvPtr)P.surv_count;
        if (FIXED && wave_id < n_trips) trips = (uint32_t)(n_trips - wave_id - 1) / (uint32_t)n_waves + 1u;
        // (the list pointer stays in two scalar registers across the loop: read from the kernarg segment once per trip like the other
        // parameters, the instruction stream of the GENERAL loop moved with it and GS_BENCH_OFFSETS=array lost 0.10 ms)
        const GsSurvPtr sl0 = FIXED ? (GsSurvPtr)P.surv_list : nullptr;
        for (int64_t t = wave_id; FIXED ? trips != 0 : t < n_trips; t += n_waves, po += po_step, trips--) {
            GsKernargPtr kp = kp0;
#ifndef GS_KERNARG_HOISTED  // (experiment, DESIGN 8.1 "kernarg re-reads": let the compiler keep the parameters live across the loop)
            asm volatile("" : "+s"(kp));
#endif
            const GsMatchParams &Q = *(const GsMatchParams *)kp;
            int64_t r = t;
            if (FIXED && sl0 != nullptr) r = (int64_t)sl0[t];
            u64 off;
            int L;
            if (FIXED) {
                // (only the mask is kept across the loop.  The length itself comes from the kernarg segment like every other parameter:
                // as a loop invariant, everything derived from it -- the clamped index, (double)max of the class-error gate -- is
                // hoisted into registers that stay live across the loop, and the kernel spills: 8 -> 36 bytes of scratch)
                L = Q.fixed_len;
                off = (u64)r * (u64)(uint32_t)L;
            } else if (Q.off_stride == 0) {  // reads of one length, back to back: nothing to load
                if (Q.surv_list != nullptr) r = (int64_t)Q.surv_list[t];
                L = Q.fixed_len;
                off = (u64)r * (u64)(uint32_t)L;
            } else {
                off = po[0];
                L = (int)(po[1] - off);
            }
            GS_STAMP(0, L)
            if (!FIXED && L - k + 1 > 128) continue;  // another kernel's: gs_classify_kernel has put it into that kernel's queue
            uint32_t pre[3];
            const uint8_t *rd = Q.seq + off;
            if (FIXED) {  // no exec-mask regions: two full words, and the third from a clamped address (inside the read) with a select
                pre[0] = rd[lane];
                pre[1] = rd[64 + lane];
                const uint32_t c2 = rd[128 + lane < L ? 128 + lane : L - 1];
                pre[2] = 128 + lane < L ? c2 : GS_FILL;
            } else {
#pragma unroll
                for (int w = 0; w < 3; w++) pre[w] = 64 * w + lane < L ? rd[64 * w + lane] : GS_FILL;
            }
            gs_process_read<false, FROM_NODES, KC, WIDE, !LDS_STATS, STRIPED, CTX, FIXED, NOGATE>(Q, st, r, off, L, lane, s_dvi, s_dcnt, wave_in_block, nullptr, nullptr, 0,
                                                                                          pre, s_g[wave_in_block], s_cur[wave_in_block], fixed_live1, t);
        }
    };
    if constexpr (CAN_FIX) {
        if (fixed_batch) {  // (wave-uniform, from the kernel's arguments)
            if constexpr (CAN_NOGATE) {
                if (nogate_batch)
                    reads(std::true_type(), std::true_type());
                else
                    reads(std::true_type(), std::false_type());
            } else
                reads(std::true_type(), std::false_type());
        } else
            reads(std::false_type(), std::false_type());
    } else
        reads(std::false_type(), std::false_type());
#if GS_PHASE
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 15) atomicAdd(&gs_phase_acc[lane], gs_phase_row()[lane]);
#endif
    if (!LDS_STATS && P.stat_recs != nullptr) {  // the rest of the wave's last chunk
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const u64 base = s_cur[wave_in_block][0], used = s_cur[wave_in_block][1];
        if (used < 64 && (u64)lane >= used) P.stat_recs[base + (u64)lane].vi = -1;
    }
    GS_STATS_EPILOGUE()
}

// ---------------------------------------------------------------------------------------------------
// Reads of 129 .. 64 NS k-mer positions in ONE trip (NS = 3: up to 192 positions, 159 .. 222 bp at k = 31, 150 bp at k < 23).  The
// long-read path takes such a read in two iterations of 128 positions, each a chain of dependent round trips (bases, gate word,
// record lines) that costs what a whole short read does however few of its positions are live: 158 bp 233 Gbp/s, 159 bp 129.  Here
// the NS sub-rounds of the read go through the probe together -- their gate words and record lines are in flight side by side --
// and the read is reduced like a short read (one pass, distinct tax ids in registers); the price is registers (planes, k-mers and
// nodes of NS sub-rounds), i.e. fewer waves per SIMD.  Same results as gs_process_read by construction: the same probe, the same
// closed forms, and every rule of matchRead (C/match/FastqKMerMatcher.java:330-531) restated for NS words of positions.
// ---------------------------------------------------------------------------------------------------
template <int NS, int KC, int CTX>
__device__ __forceinline__ void gs_process_read_wide(const GsMatchParams &P, const GsStats &st, int64_t r, u64 off, int L, int lane, uint32_t *wave_g) {
    // (the list of distinct tax ids goes through the wave's rows when the threshold rule needs it in memory: the probe is through with them)
    int *s_dvi = reinterpret_cast<int *>(wave_g), *s_dcnt = reinterpret_cast<int *>(wave_g) + 64 * NS;
    static_assert(GS_WIDE_WORDS(NS) >= 2 * 64 * NS, "room for the list");
    const GsDbDev &db = P.db;
    const int k = KC ? KC : db.k;
    const int max = L - k + 1;
    const uint8_t *rd = P.seq + off;
    int out_class = -1, out_flags = 0;
    if (max > 0) {
        const u64 key_lo = ((1ULL << 40) - 1) - ((u64)(P.first_read_no + r) & ((1ULL << 40) - 1));
        u64 Bhi[NS + 1], Blo[NS + 1], Bbad[NS + 1];
#pragma unroll
        for (int w = 0; w <= NS; w++) gs_load_word(rd, L, w, lane, Bhi[w], Blo[w], Bbad[w]);
        int bad_lo = 0;
        bool bad_hi = false;
        {   // bad-base census for the closed form of the INVALID steps (as gs_process_read; every word belongs to this one trip)
            const int q = max - 1;
#pragma unroll
            for (int w = 0; w <= NS; w++) {
                const int lo_bits = q - 64 * w;
                const u64 m_lo = lo_bits >= 64 ? ~0ULL : (lo_bits <= 0 ? 0ULL : ((1ULL << lo_bits) - 1));
                bad_lo += __popcll(Bbad[w] & m_lo);
                bad_hi = bad_hi || ((Bbad[w] & ~m_lo) != 0);
            }
        }
        int node[NS];
        const GsMark mk = {P.count_unique, P.hit_counts, nullptr, nullptr};
        gs_probe_planes<KC, false, CTX, false, NS>(db, Bhi, Blo, Bbad, 0, max, lane, node, wave_g, mk);
        u64 hit[NS], any_hit = 0;
        int n_miss = 0;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            hit[s] = __ballot(node[s] >= 0);
            any_hit |= hit[s];
            n_miss += __popcll(__ballot(node[s] == GS_NODE_MISS));
        }
        if (any_hit != 0) {
            out_flags = GS_F_FOUND | GS_F_RETURNED;
            // ---- contigs (:390-413, :455-473): a lane that starts a run of a hit node books it; the run ends at the next change of
            // node, in its own word or a later one, or with the read
            u64 chg[NS];
#pragma unroll
            for (int s = 0; s < NS; s++) {
                const int up = __shfl_up(node[s], 1);
                int before = GS_NODE_NONE;  // (in front of position 0: nothing -- the first position starts a run)
                if (s > 0) before = gs_readlane(node[s - 1], 63);
                const int prev = lane == 0 ? before : up;
                const int nvs = max - 64 * s;
                const u64 vm = nvs >= 64 ? ~0ULL : (nvs <= 0 ? 0ULL : ((1ULL << nvs) - 1ULL));
                chg[s] = __ballot(node[s] != prev) & vm;
            }
            int later = max;  // first change in the words behind the current one (or the read's end)
#pragma unroll
            for (int s = NS - 1; s >= 0; s--) {
                const u64 above = (chg[s] >> 1) >> lane;
                const int end = above ? 64 * s + lane + 1 + __builtin_ctzll(above) : later;
                if (GS_ACT(hit[s] & chg[s])) st.contig(node[s], end - (64 * s + lane), key_lo);
                if (chg[s]) later = 64 * s + __builtin_ctzll(chg[s]);
            }
            // ---- the distinct hit nodes in order of first appearance: reads1KMer (:434-439), mergeReadTaxidPath (:568-586); entry i
            // of the list (node, votes) lives in lane i & 63 of register set i >> 6
            int dvi[NS], dcnt[NS], nd = 0;
            int path = -1, ptin = 0, ptout = 0, used = 0;
#pragma unroll
            for (int h = 0; h < NS; h++) {
                dvi[h] = -1;
                dcnt[h] = 0;
            }
            u64 m[NS];
#pragma unroll
            for (int s = 0; s < NS; s++) m[s] = hit[s];
            for (;;) {
                int j = -1;
#pragma unroll
                for (int s = NS - 1; s >= 0; s--)
                    if (m[s]) j = 64 * s + __builtin_ctzll(m[s]);
                if (j < 0) break;
                int nvj = 0;
#pragma unroll
                for (int s = 0; s < NS; s++)
                    if ((j >> 6) == s) nvj = gs_readlane(node[s], j & 63);
                int c = 0;
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    const u64 e = __ballot(node[s] == nvj);
                    c += __popcll(e);
                    m[s] &= ~e;
                }
#pragma unroll
                for (int h = 0; h < NS; h++)
                    if ((nd >> 6) == h && lane == (nd & 63)) {
                        dvi[h] = nvj;
                        dcnt[h] = c;
                    }
                nd++;
                if (lane == 0) st.add(nvj, GS_S_READS_1KMER, 1);
                if (P.classify) {
                    const int ntin = st.tin[nvj], ntout = st.tout[nvj];
                    const bool mine = lane < used;
                    const bool a = mine && gs_anc_or_self(ptin, ptout, ntin);  // path anc-or-self of node
                    const bool b = mine && gs_anc_or_self(ntin, ntout, ptin);  // node anc-or-self of path
                    const u64 rel = __ballot(a || b);
                    if (rel) {
                        if (lane == __builtin_ctzll(rel) && a) {
                            path = nvj;
                            ptin = ntin;
                            ptout = ntout;
                        }
                    } else if (used < P.max_paths) {
                        if (lane == used) {
                            path = nvj;
                            ptin = ntin;
                            ptout = ntout;
                        }
                        used++;
                    }
                }
            }
            // ---- classification (:474-531)
            if (P.classify) {
                const int tax_err = n_miss + bad_lo + (bad_hi ? 1 : 0);
                const double mt = P.max_read_tax_err;
                const bool disabled = mt >= 0 && ((mt >= 1 && (double)tax_err > mt) || ((double)tax_err > mt * (double)max));
                if (!disabled) {
                    int cn = -1, first_node = -1, best = 0;
                    // sumCounts per candidate path (SmallTaxTree.java:184-193): lanes = paths
                    int sum = 0;
                    for (int dd = 0; dd < nd; dd++) {
                        int v = 0, c = 0;
#pragma unroll
                        for (int h = 0; h < NS; h++)
                            if ((dd >> 6) == h) {
                                v = gs_readlane(dvi[h], dd & 63);
                                c = gs_readlane(dcnt[h], dd & 63);
                            }
                        if (lane < used && gs_anc_or_self(st.tin[v], st.tout[v], ptin)) sum += c;
                    }
                    u64 tie_mask = 0;  // max + ties exactly as the in-place scan (:476-487); tie order = path order
                    for (int i = 0; i < used; i++) {
                        const int si = gs_readlane(sum, i);
                        if (si > best) {
                            best = si;
                            tie_mask = 0;
                        }
                        if (si >= best) tie_mask |= 1ULL << i;
                    }
                    int cand = path;
                    if (P.threshold > 1) {  // lowestNodeWhereSumAboveThreshold per tied path (SmallTaxTree.java:208-221)
#pragma unroll
                        for (int h = 0; h < NS; h++) {
                            s_dvi[64 * h + lane] = dvi[h];
                            s_dcnt[64 * h + lane] = dcnt[h];
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        int mapped = -1;
                        if ((tie_mask >> lane) & 1ULL) {
                            int acc = 0;
                            for (int x = path; x >= 0 && mapped < 0; x = st.parent[x])
                                for (int dd = 0; dd < nd; dd++)
                                    if (s_dvi[dd] == x) {
                                        acc += s_dcnt[dd];
                                        if (acc >= P.threshold) mapped = x;
                                    }
                        }
                        cand = mapped;
                        __builtin_amdgcn_wave_barrier();
                    }
                    {
                        bool first = true;
                        for (u64 tm = tie_mask; tm; tm &= tm - 1) {
                            const int x = gs_readlane(cand, __builtin_ctzll(tm));
                            if (first) {
                                cn = x;
                                first_node = x;
                                first = false;
                            } else
                                cn = gs_lca(st, cn, x);
                        }
                    }
                    out_class = cn;
                    if (cn < 0) {
                        out_flags &= ~GS_F_RETURNED;  // "return false" (:497-500)
                    } else {
                        int read_kmers = best;
                        if (P.threshold > 1) {  // sumCounts(readTaxIdNode[0]) after the promotion (:506-507)
                            read_kmers = 0;
                            const int ft = st.tin[first_node];
                            for (int dd = 0; dd < nd; dd++) {
                                int v = 0, c = 0;
#pragma unroll
                                for (int h = 0; h < NS; h++)
                                    if ((dd >> 6) == h) {
                                        v = gs_readlane(dvi[h], dd & 63);
                                        c = gs_readlane(dcnt[h], dd & 63);
                                    }
                                if (gs_anc_or_self(st.tin[v], st.tout[v], ft)) read_kmers += c;
                            }
                        }
                        const int class_err = max - read_kmers;
                        const double mc = P.max_read_class_err;
                        if (mc < 0 || (mc >= 1 && (double)class_err <= mc) || ((double)class_err <= mc * (double)max)) {
                            out_flags |= GS_F_COUNTED;
                            if (lane == 0) {
                                const double err = (double)tax_err / (double)max;
                                const double cerr = (double)class_err / (double)max;
                                st.add(cn, GS_S_READS, 1);
                                st.add(cn, GS_S_READS_KMERS, (u64)read_kmers);
                                st.add(cn, GS_S_READS_BPS, (u64)L);
                                st.dadd(cn, GS_D_ERR_SUM, err);
                                st.dadd(cn, GS_D_ERR_SQ_SUM, err * err);
                                st.dadd(cn, GS_D_CLASS_ERR_SUM, cerr);
                                st.dadd(cn, GS_D_CLASS_ERR_SQ_SUM, cerr * cerr);
                            }
                        }
                    }
                }
            }
        }
    }
    if (lane == 0) {
        if (P.class_vi) P.class_vi[r] = out_class;
        if (P.flags) P.flags[r] = (uint8_t)out_flags;
    }
}

// waves per SIMD, three sub-rounds: 8 (64 VGPRs, a few spilled) beats 7 / 6 (80 VGPRs, none spilled) / 5 / 4 on reads of 159, 190
// and 222 bp -- 168 / 168 / 161 / 149 / 105 Gbp/s at 159 bp; four sub-rounds: 6 beats 8 / 7 / 5 -- 196 / 169 / 189 / 179 Gbp/s at
// 250 bp (the long-read path: 180)
#ifndef GS_WIDE_WAVES
#define GS_WIDE_WAVES 8
#endif
#ifndef GS_WIDE4_WAVES
#define GS_WIDE4_WAVES 6
#endif
#ifndef GS_WIDE_ANYK_WAVES  // (k as a run-time value; a store without records keeps half a bucket line per sub-round in registers: k = 16 table-only 112.6 Gbp/s at 7, 91.8 at 8, 112.0 at 6; a k = 25 record store: 7 = 8 > 6)
#define GS_WIDE_ANYK_WAVES 7
#endif
#define GS_WIDE_WAVES_OF(NS, KC) ((NS) == 4 ? GS_WIDE4_WAVES : ((KC) ? GS_WIDE_WAVES : GS_WIDE_ANYK_WAVES))
// The reads of queue NS - 2 (filled by gs_match_kernel: 129 .. 192 positions in queue 1, 193 .. 256 in queue 2, GsMatchParams::
// wide_mask), or -- long_list == nullptr: reads of one length, gs_match_submit_fixed, the launcher has looked -- every read of the batch.
template <bool LDS_STATS, int NS, int KC>
__global__ __launch_bounds__(GS_BLOCK) __attribute__((amdgpu_waves_per_eu(GS_WIDE_WAVES_OF(NS, KC), GS_WIDE_WAVES_OF(NS, KC)))) void gs_match_wide_kernel(GsMatchParams P) {
    const bool all = P.long_list == nullptr;
    unsigned int *qc = P.long_count + 2 * (NS - 2);  // [0] entries, [1] the cursor the waves draw chunks of GS_LONG_CHUNK entries from
    if (!all && qc[0] == 0) return;
    GS_STATS_PROLOGUE()
    __shared__ __attribute__((aligned(8))) uint32_t s_g[GS_BLOCK / 64][GS_WIDE_WORDS(NS)];
    const int lane = gs_lane();
    const int wave_in_block = gs_rfl((int)(threadIdx.x >> 6));
    const u64 n_q = all ? (u64)P.n_reads : (u64)qc[0];
    const uint32_t *list = all ? nullptr : P.long_list + (size_t)(NS - 2) * (size_t)P.long_cap;
    for (;;) {
        __builtin_amdgcn_wave_barrier();  // (as gs_match_long_kernel: no lane-0 test threaded through the back edge)
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(qc + 1, 1u);
        c = (uint32_t)gs_rfl((int)c);
        if ((u64)c * GS_LONG_CHUNK >= n_q) break;
        const u64 at = (u64)c * GS_LONG_CHUNK + (u64)lane;
        const uint32_t mine = at < n_q ? (all ? (uint32_t)at : list[at]) : GS_LONG_NONE;
        // the offsets of the chunk's reads with one gather (every lane its own read's), not one dependent load per read
        u64 my_off = 0;
        int my_len = 0;
        if (P.off_stride != 0 && mine != GS_LONG_NONE) {
            const uint64_t *po = P.off + (int64_t)mine * P.off_stride;
            my_off = po[0];
            my_len = (int)(po[1] - my_off);
        }
        for (u64 todo = __ballot(mine != GS_LONG_NONE); todo; todo &= todo - 1) {
            const int i = __builtin_ctzll(todo);
            const int64_t r = (int64_t)(uint32_t)gs_readlane((int)mine, i);
            u64 off;
            int L;
            if (P.off_stride == 0) {
                L = P.fixed_len;
                off = (u64)r * (u64)(uint32_t)L;
            } else {
                off = ((u64)(uint32_t)gs_readlane((int)(my_off >> 32), i) << 32) | (u64)(uint32_t)gs_readlane((int)(uint32_t)my_off, i);
                L = gs_readlane(my_len, i);
            }
            gs_process_read_wide<NS, KC, 2>(P, st, r, off, L, lane, s_g[wave_in_block]);
        }
    }
    GS_STATS_EPILOGUE()
}

// waves per SIMD of the long-read kernel: left alone the compiler takes 80-90 VGPRs (5 waves); at 8 waves (64 VGPRs, 8 of them
// spilled) reads of 1000 bp run at 162 instead of 134 Gbp/s, at 6 waves (77 VGPRs, no spills) at 140 (tools/long_read_rate.py)
#ifndef GS_LONG_WAVES
#define GS_LONG_WAVES GS_WAVES
#endif
#if GS_LONG_WAVES
#define GS_LONG_ATTR __attribute__((amdgpu_waves_per_eu(GS_LONG_WAVES, GS_LONG_WAVES)))
#else
#define GS_LONG_ATTR
#endif
template <bool LDS_STATS, bool FROM_NODES, bool WIDE = false, bool STRIPED = false, int KC = 0>
__global__ __launch_bounds__(GS_BLOCK) GS_LONG_ATTR void gs_match_long_kernel(GsMatchParams P, int32_t *scratch, uint32_t *serials) {
    // long_list == nullptr: EVERY read of the batch is a long one (reads of one length, gs_match_submit_fixed: the launcher has looked) --
    // no queue was written, chunk c holds the reads 64 c .. 64 c + 63
    const bool all_long = P.long_list == nullptr;
    if (!all_long && P.long_count[0] == 0) return;  // (a batch of short reads: nothing queued, no counters to set up and flush)
    GS_STATS_PROLOGUE()
    const int lane = gs_lane();
    const int wave_in_block = gs_rfl((int)(threadIdx.x >> 6));  // wave-uniform: per-read bookkeeping runs on the scalar unit
    const int64_t wave_id = (int64_t)blockIdx.x * (GS_BLOCK / 64) + wave_in_block;
    __shared__ __attribute__((aligned(8))) uint32_t s_g[GS_BLOCK / 64][2 * GS_ROW + (STRIPED ? GS_STRIPE_WORDS : 0)];
    GS_STRIPE_TABLE(&P)
    // The queue (written by gs_classify_kernel on the same stream) is a dense list; the waves of this kernel draw chunks of
    // GS_LONG_CHUNK entries from a shared cursor
    // (long_count[1]) until the queue is empty: reads of very different lengths spread over the waves by themselves, and
    // every wave leaves the loop with the first chunk index beyond the end.
    const u64 n_long = all_long ? (u64)P.n_reads : (u64)P.long_count[0];
    // per-wave vote rows (tag = serial of the read that last touched a node, cnt = its votes in that read): in LDS for the
    // taxonomies whose counters are in LDS as well (every distinct node of every iteration reads and writes them: two
    // dependent round trips to HBM otherwise), else this wave's rows of `scratch`, which persist from launch to launch
    __shared__ int32_t s_votes[LDS_STATS ? GS_BLOCK / 64 : 1][LDS_STATS ? 2 * GS_NV_LDS : 1];
    int32_t *tag = LDS_STATS ? s_votes[wave_in_block] : scratch + (size_t)wave_id * 2 * (size_t)nv;
    int32_t *cnt = tag + (LDS_STATS ? GS_NV_LDS : nv);
    uint32_t serial = LDS_STATS ? 0u : serials[wave_id];
    if (LDS_STATS) {
        for (int i = lane; i < GS_NV_LDS; i += 64) tag[i] = 0;  // (serials start at 1)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    for (;;) {
        // (keeps the compiler from threading a lane-0 test at the end of an iteration into this one through the back edge: lane 0
        // and the other lanes would go around the loop separately and read their own `c` -- seen in gs_inflate_dev.hip)
        __builtin_amdgcn_wave_barrier();
        uint32_t c = 0;
        if (lane == 0) c = atomicAdd(P.long_count + 1, 1u);
        c = (uint32_t)gs_rfl((int)c);
        if ((u64)c * GS_LONG_CHUNK >= n_long) break;
        const u64 at = (u64)c * GS_LONG_CHUNK + (u64)lane;
        const uint32_t mine = at < n_long ? (all_long ? (uint32_t)at : P.long_list[at]) : GS_LONG_NONE;  // (the queue is a dense list)
        for (u64 todo = __ballot(mine != GS_LONG_NONE); todo; todo &= todo - 1) {
            serial++;
            if (serial == 0) {  // wrap after 2^32 - 1 long reads on this wave: old tags could alias, so the wave's tag row starts over
                for (int i = lane; i < nv; i += 64) gs_sc_store(tag + i, 0);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
                serial = 1;
            }
            const int64_t r = (int64_t)(uint32_t)gs_readlane((int)mine, __builtin_ctzll(todo));
            u64 off;
            int L;
            if (P.off_stride == 0) {
                L = P.fixed_len;
                off = (u64)r * (u64)(uint32_t)L;
            } else {
                const uint64_t *po = P.off + r * P.off_stride;
                off = po[0];
                L = (int)(po[1] - off);
            }
            const uint32_t none[3] = {0, 0, 0};
            gs_process_read<true, FROM_NODES, KC, WIDE, false, STRIPED>(P, st, r, off, L, lane, nullptr, nullptr, wave_in_block, tag,
                                                       cnt, (int)serial, none, s_g[wave_in_block], nullptr);
        }
    }
    if (!LDS_STATS && lane == 0) serials[wave_id] = serial;
    GS_STATS_EPILOGUE()
}

// ---------------------------------------------------------------------------------------------------
// Reads of GS_HUGE_MIN positions and more, over many waves (a chromosome on ONE wave runs at 30 Mbp/s).
// A read is cut into chunks of whole iterations (GS_HUGE_CHUNK_MIN positions and more, at most GS_HUGE_MAX_CHUNKS chunks); gs_match_huge_kernel gives every chunk a
// wave, which walks it exactly as the long-read path walks a read -- same probe, same closed form for windows with a bad base, the
// contigs INSIDE the chunk booked by the lanes that start them -- and leaves behind what a single wave would have carried across:
//   * per read and node, atomically: the positions that hold the node (the votes) and the FIRST of them;
//   * per read: misses, bad bases, "some k-mer hit";
//   * per chunk: the run it starts with and the run that is open at its end (neither is booked: a run may span chunks).
// gs_match_huge_finish_kernel, one wave per read, then does what is sequential in matchRead and cheap: closes the runs across the
// seams (FastqKMerMatcher.java:390-413, :455-473), walks the distinct nodes in order of first appearance -- reads1KMer (:434-439),
// mergeReadTaxidPath (:568-586) --, classifies (:474-531) from the vote counts, and clears the read's rows for the next batch.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int gs_huge_chunk_positions(int max, int chunk_min) {
    int c = ((max + GS_HUGE_MAX_CHUNKS - 1) / GS_HUGE_MAX_CHUNKS + 127) & ~127;
    return c < chunk_min ? chunk_min : c;
}

__device__ __forceinline__ void gs_huge_read(const GsMatchParams &P, int64_t r, u64 &off, int &L) {
    if (P.off_stride == 0) {
        L = P.fixed_len;
        off = (u64)r * (u64)(uint32_t)L;
    } else {
        const uint64_t *po = P.off + r * P.off_stride;
        off = po[0];
        L = (int)(po[1] - off);
    }
}

// votes of one node from one chunk into the read's rows; the wave that brings the first ones puts the node on the read's list
__device__ __forceinline__ void gs_huge_vote(uint32_t *cnt, uint32_t *first, uint32_t *touch, GsHugeHead *h0, int v, uint32_t c, uint32_t pos) {
    if (atomicAdd(cnt + v, c) == 0) touch[atomicAdd(&h0->n_touch, 1u)] = (uint32_t)v;  // (once per copy: the list may hold a node several times)
    atomicMin(first + v, pos);
}

// (waves per SIMD: a chunk is a chain of dependent iterations, and a spilled register is a round trip to memory inside it)
#ifndef GS_HUGE_WAVES
#define GS_HUGE_WAVES GS_LONG_WAVES
#endif
#if GS_HUGE_WAVES
#define GS_HUGE_ATTR __attribute__((amdgpu_waves_per_eu(GS_HUGE_WAVES, GS_HUGE_WAVES)))
#else
#define GS_HUGE_ATTR
#endif
template <bool LDS_STATS, bool STRIPED, int KC = 0>
__global__ __launch_bounds__(GS_BLOCK) GS_HUGE_ATTR void gs_match_huge_kernel(GsMatchParams P) {
    const unsigned int n_huge_all = P.huge_count[0];
    if (n_huge_all == 0) return;
    const int n_huge = (int)(n_huge_all < (unsigned int)P.huge_slots ? n_huge_all : (unsigned int)P.huge_slots);
    GS_STATS_PROLOGUE()
    const int lane = gs_lane();
    const int wave_in_block = gs_rfl((int)(threadIdx.x >> 6));
    const int64_t wave_id = (int64_t)blockIdx.x * (GS_BLOCK / 64) + wave_in_block;
    const int64_t n_waves = (int64_t)gridDim.x * (GS_BLOCK / 64);
    __shared__ __attribute__((aligned(8))) uint32_t s_g[GS_BLOCK / 64][2 * GS_ROW + (STRIPED ? GS_STRIPE_WORDS : 0)];
    GS_STRIPE_TABLE(&P)
    uint32_t *wave_g = s_g[wave_in_block];
    const GsDbDev &db = P.db;
    const int k = KC ? KC : db.k;
    const GsMark mk = {P.count_unique, P.hit_counts, STRIPED ? P.bitmap : nullptr, STRIPED ? P.bitmap + ((db.bucket_mask + 1) * GS_SLOTS_PER_BUCKET >> 5) : nullptr};
    // the chunks of all reads in one row: s_first[slot] = number of the read's first chunk (GS_HUGE_SLOTS = GS_BLOCK: a thread per slot)
    __shared__ int s_first[GS_HUGE_SLOTS + 1];
    {
        int mine = 0;
        if ((int)threadIdx.x < n_huge) {
            u64 off;
            int L;
            gs_huge_read(P, (int64_t)P.huge_list[threadIdx.x], off, L);
            const int max = L - k + 1, C = gs_huge_chunk_positions(max, P.huge_chunk_min);
            mine = (max + C - 1) / C;
        }
        s_first[threadIdx.x + 1] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            int sum = 0;
            s_first[0] = 0;
            for (int i = 1; i <= n_huge; i++) s_first[i] = (sum += s_first[i]);
        }
        __syncthreads();
    }
    const int n_all = s_first[n_huge];
    for (int64_t g = wave_id; g < n_all; g += n_waves) {
        int slot = 0;
        {   // the last slot whose first chunk is <= g (reads have at least one chunk each)
            int lo = 0, hi = n_huge - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_first[mid] <= (int)g)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            slot = gs_rfl(lo);
        }
        const int c = (int)g - s_first[slot];
        const int64_t r = (int64_t)P.huge_list[slot];
        u64 off;
        int L;
        gs_huge_read(P, r, off, L);
        const int max = L - k + 1;
        const uint8_t *rd = P.seq + off;
        const int C = gs_huge_chunk_positions(max, P.huge_chunk_min);
        const int n_iter_all = (max + 127) >> 7;
        const u64 key_lo = ((1ULL << 40) - 1) - ((u64)(P.first_read_no + r) & ((1ULL << 40) - 1));
        // (GS_HUGE_COPIES copies of the read's rows and counters, chunk c on copy c mod GS_HUGE_COPIES: the chunks of a chromosome vote
        // for the same handful of tax ids, and atomics on ONE address execute one after the other -- 4 883 chunks x 2 atomics per tax id
        // were most of the kernel's 0.17 ms; the finish kernel folds the copies)
        const size_t copy = (size_t)(c & (GS_HUGE_COPIES - 1)), row = ((size_t)slot * GS_HUGE_COPIES + copy) * (size_t)nv;
        uint32_t *cnt = P.huge_cnt + row, *first = P.huge_first + row;
        uint32_t *touch = P.huge_touch + (size_t)slot * GS_HUGE_COPIES * (size_t)nv;
        GsHugeHead *h = P.huge_head + (size_t)slot * GS_HUGE_COPIES + copy;
        GsHugeHead *h0 = P.huge_head + (size_t)slot * GS_HUGE_COPIES;  // (the touch list's length lives in copy 0)
        const int p0 = c * C, p1 = p0 + C < max ? p0 + C : max;
        int carry_last = GS_NODE_NONE, cur_start = p0, head_node = GS_NODE_NONE, head_len = 0;
        bool head_open = true, found = false, bad_hi = false;
        int n_miss = 0, bad_lo = 0;
        // the chunk's votes per node, one node per lane (a chunk of a genome meets a handful; the 65th goes to the rows at once)
        int c_node = -1, n_cached = 0;
        uint32_t c_cnt = 0, c_first = 0;
        for (int it = p0 >> 7; it < (p1 + 127) >> 7; it++) {
            const int base = it << 7;
            u64 Bhi[3], Blo[3], Bbad[3];
#pragma unroll
            for (int w = 0; w < 3; w++) gs_load_word(rd, L, 2 * it + w, lane, Bhi[w], Blo[w], Bbad[w]);
            {   // bad-base census as gs_process_read: words 2 it and 2 it + 1 belong to this iteration, word 2 it + 2 to the read's last
                const int q = max - 1;
                const int nw = (it == n_iter_all - 1) ? 3 : 2;
#pragma unroll
                for (int w = 0; w < 3; w++) {
                    if (w < nw) {
                        const int lo_bits = q - (base + 64 * w);
                        const u64 m_lo = lo_bits >= 64 ? ~0ULL : (lo_bits <= 0 ? 0ULL : ((1ULL << lo_bits) - 1));
                        bad_lo += __popcll(Bbad[w] & m_lo);
                        bad_hi = bad_hi || ((Bbad[w] & ~m_lo) != 0);
                    }
                }
            }
            int node[2];
            // (the marks of first-seen k-mers as ONE atomic per record line: a chromosome of the store's own species is nothing but
            // first-seen k-mers -- 5 M device-scope atomics, each a request to the fabric, were 0.09 of the chunk kernel's 0.13 ms)
            gs_probe_planes<KC, STRIPED, 2, true>(db, Bhi, Blo, Bbad, base, max, lane, node, wave_g, mk);
            const u64 hit0 = __ballot(node[0] >= 0), hit1 = __ballot(node[1] >= 0);
            found = found || ((hit0 | hit1) != 0);
            n_miss += __popcll(__ballot(node[0] == GS_NODE_MISS)) + __popcll(__ballot(node[1] == GS_NODE_MISS));
            if (base == p0) {  // the chunk's first position opens its head run (no change in front of it)
                carry_last = gs_readlane(node[0], 0);
                head_node = carry_last;
            }
            int prev[2];
            {
                const int up0 = __shfl_up(node[0], 1);
                const int up1 = __shfl_up(node[1], 1);
                const int last0 = gs_readlane(node[0], 63);
                prev[0] = lane == 0 ? carry_last : up0;
                prev[1] = lane == 0 ? last0 : up1;
            }
            const int nv0 = max - base, nv1 = max - base - 64;
            const u64 vm0 = nv0 >= 64 ? ~0ULL : (nv0 <= 0 ? 0ULL : ((1ULL << nv0) - 1ULL));
            const u64 vm1 = nv1 >= 64 ? ~0ULL : (nv1 <= 0 ? 0ULL : ((1ULL << nv1) - 1ULL));
            const u64 chg0 = __ballot(node[0] != prev[0]) & vm0;
            const u64 chg1 = __ballot(node[1] != prev[1]) & vm1;
            if ((chg0 | chg1) != 0) {  // the run that was open ends at the first change
                const int q = chg0 ? __builtin_ctzll(chg0) : 64 + __builtin_ctzll(chg1);
                if (head_open) {
                    head_len = base + q - p0;
                    head_open = false;
                } else if (carry_last >= 0 && lane == 0)
                    st.contig(carry_last, base + q - cur_start, key_lo);
            }
            {   // hit contigs that start at a change of this iteration and end before the iteration does
                const u64 a0 = (chg0 >> 1) >> lane, a1 = (chg1 >> 1) >> lane;
                const int e1 = chg1 ? 64 + __builtin_ctzll(chg1) : -1;
                const int end0 = a0 ? lane + 1 + __builtin_ctzll(a0) : e1;
                const int end1 = a1 ? 64 + lane + 1 + __builtin_ctzll(a1) : -1;
                const u64 c0m = hit0 & chg0 & (chg1 ? ~0ULL : (chg0 ? (1ULL << (63 - __builtin_clzll(chg0))) - 1ULL : 0ULL));
                const u64 c1m = hit1 & chg1 & (chg1 ? (1ULL << (63 - __builtin_clzll(chg1))) - 1ULL : 0ULL);
                if (GS_ACT(c0m)) st.contig(node[0], end0 - lane, key_lo);
                if (GS_ACT(c1m)) st.contig(node[1], end1 - 64 - lane, key_lo);
            }
            if (chg1)
                cur_start = base + 127 - __builtin_clzll(chg1);
            else if (chg0)
                cur_start = base + 63 - __builtin_clzll(chg0);
            // the distinct hit nodes of this iteration
            u64 m0 = hit0, m1 = hit1;
            while ((m0 | m1) != 0) {
                const int j = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1);
                const int nvj = j < 64 ? gs_readlane(node[0], j) : gs_readlane(node[1], j - 64);
                const u64 e0 = __ballot(node[0] == nvj), e1 = __ballot(node[1] == nvj);
                m0 &= ~e0;
                m1 &= ~e1;
                const uint32_t votes = (uint32_t)(__popcll(e0) + __popcll(e1));
                const u64 has = __ballot(c_node == nvj);
                if (has) {
                    if (lane == __builtin_ctzll(has)) c_cnt += votes;
                } else if (n_cached < 64) {
                    if (lane == n_cached) {
                        c_node = nvj;
                        c_cnt = votes;
                        c_first = (uint32_t)(base + j);
                    }
                    n_cached++;
                } else if (lane == 0)
                    gs_huge_vote(cnt, first, touch, h0, nvj, votes, (uint32_t)(base + j));
            }
            {
                const int last_p = (max - 1 < base + 127) ? max - 1 : base + 127;
                const int ls = (last_p - base) >> 6, ll = (last_p - base) & 63;
                carry_last = gs_readlane(ls ? node[1] : node[0], ll);
            }
        }
        if (c_node >= 0) gs_huge_vote(cnt, first, touch, h0, c_node, c_cnt, c_first);
        if (lane == 0) {
            GsHugeChunk rec;
            rec.head_node = head_node;
            rec.head_len = head_open ? p1 - p0 : head_len;
            rec.tail_node = head_open ? head_node : carry_last;
            rec.tail_len = head_open ? -1 : p1 - cur_start;
            P.huge_chunks[(size_t)slot * GS_HUGE_MAX_CHUNKS + (size_t)c] = rec;
            if (n_miss) atomicAdd(&h->n_miss, (unsigned int)n_miss);
            if (bad_lo) atomicAdd(&h->bad_lo, (unsigned int)bad_lo);
            if (found || bad_hi) atomicOr(&h->flags, (found ? 1u : 0u) | (bad_hi ? 2u : 0u));
        }
    }
    GS_STATS_EPILOGUE()
}

template <bool LDS_STATS>
__global__ __launch_bounds__(GS_BLOCK) void gs_match_huge_finish_kernel(GsMatchParams P) {
    const unsigned int n_huge_all = P.huge_count[0];
    if (n_huge_all == 0) return;
    const int n_huge = (int)(n_huge_all < (unsigned int)P.huge_slots ? n_huge_all : (unsigned int)P.huge_slots);
    GS_STATS_PROLOGUE()
    const int lane = gs_lane();
    const int wave_in_block = gs_rfl((int)(threadIdx.x >> 6));
    const int slot = (int)blockIdx.x * (GS_BLOCK / 64) + wave_in_block;
    if (slot < n_huge) {
        const GsDbDev &db = P.db;
        const int k = db.k;
        const int64_t r = (int64_t)P.huge_list[slot];
        u64 off;
        int L;
        gs_huge_read(P, r, off, L);
        const int max = L - k + 1;
        const int C = gs_huge_chunk_positions(max, P.huge_chunk_min);
        const int n_chunks = (max + C - 1) / C;
        const u64 key_lo = ((1ULL << 40) - 1) - ((u64)(P.first_read_no + r) & ((1ULL << 40) - 1));
        uint32_t *cnt_c = P.huge_cnt + (size_t)slot * GS_HUGE_COPIES * (size_t)nv, *first_c = P.huge_first + (size_t)slot * GS_HUGE_COPIES * (size_t)nv;
        uint32_t *touch = P.huge_touch + (size_t)slot * GS_HUGE_COPIES * (size_t)nv;
        uint32_t *cnt = P.huge_fold + (size_t)slot * 2 * (size_t)nv, *first = cnt + nv;  // the copies folded: votes and first position per node
        GsHugeHead *hd = P.huge_head + (size_t)slot * GS_HUGE_COPIES;
        unsigned int hflags = 0, h_miss = 0, h_bad = 0;
        if (lane < GS_HUGE_COPIES) {
            hflags = hd[lane].flags;
            h_miss = hd[lane].n_miss;
            h_bad = hd[lane].bad_lo;
        }
#pragma unroll
        for (int o = GS_HUGE_COPIES / 2; o >= 1; o >>= 1) {
            hflags |= (unsigned int)__shfl_xor((int)hflags, o);
            h_miss += (unsigned int)__shfl_xor((int)h_miss, o);
            h_bad += (unsigned int)__shfl_xor((int)h_bad, o);
        }
        hflags = (unsigned int)gs_rfl((int)hflags);
        const bool found = (hflags & 1u) != 0;
        const int tax_err = gs_rfl((int)h_miss) + gs_rfl((int)h_bad) + ((hflags & 2u) ? 1 : 0);
        const int n_touch = (int)hd[0].n_touch;
        for (int i = lane; i < n_touch; i += 64) {  // (a node that is on the list twice is folded twice, to the same values)
            const int v = (int)touch[i];
            uint32_t total = 0, fmin = 0xffffffffu;
            uint32_t cv[GS_HUGE_COPIES], fv[GS_HUGE_COPIES];  // (all loads on their way before the first is waited for)
#pragma unroll
            for (int cp = 0; cp < GS_HUGE_COPIES; cp++) {
                cv[cp] = cnt_c[(size_t)cp * nv + v];
                fv[cp] = first_c[(size_t)cp * nv + v];
            }
#pragma unroll
            for (int cp = 0; cp < GS_HUGE_COPIES; cp++) {
                total += cv[cp];
                fmin = fv[cp] < fmin ? fv[cp] : fmin;
            }
            cnt[v] = total;
            first[v] = fmin;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int out_class = -1, out_flags = 0;
        // ---- the runs across the seams, 64 chunks at a time, one per lane.  With link(c) = "chunk c starts with the node chunk c - 1
        // ends with" and whole(c) = "no change inside c", the length of the run that is open at the end of chunk c is
        //     out(c) = whole(c) && link(c) ? out(c - 1) + head_len(c) : (whole(c) ? head_len(c) : tail_len(c))
        // -- a segmented sum --, the run that is open at the end of c - 1 is closed at the seam if !link(c) (length out(c - 1)), and the
        // head run of c is closed inside c if !whole(c) (length head_len(c), plus out(c - 1) if link(c)).
        {
            const GsHugeChunk *ch = P.huge_chunks + (size_t)slot * GS_HUGE_MAX_CHUNKS;
            int carry_node = GS_NODE_NONE, carry_out = 0;  // tail node and out() of the chunk before this round's first
            const GsHugeChunk none = {GS_NODE_NONE, 0, GS_NODE_NONE, -1};
            GsHugeChunk next = lane < n_chunks ? ch[lane] : none;
            for (int c0 = 0; c0 < n_chunks; c0 += 64) {
                const bool valid = c0 + lane < n_chunks;
                const GsHugeChunk mine = next;
                next = c0 + 64 + lane < n_chunks ? ch[c0 + 64 + lane] : none;  // (on its way while this round is booked)
                const int up_node = __shfl_up(mine.tail_node, 1);
                const int prev_node = lane == 0 ? carry_node : up_node;
                const bool link = valid && (c0 + lane > 0) && mine.head_node == prev_node;
                const bool whole = mine.tail_len < 0;
                // segmented inclusive sum: a lane that does not continue its predecessor's run starts a segment
                int val = whole ? mine.head_len : mine.tail_len;
                bool cont = whole && link;  // "my value is added to the one before me"
                if (lane == 0 && cont) {
                    val += carry_out;
                    cont = false;
                }
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int pv = __shfl_up(val, d);
                    const int pc = __shfl_up((int)cont, d);
                    if (lane >= d && cont) {
                        val += pv;
                        cont = pc != 0;
                    }
                }
                const int up_out = __shfl_up(val, 1);
                const int prev_out = lane == 0 ? carry_out : up_out;
                if (valid && c0 + lane > 0 && !link && prev_node >= 0) st.contig(prev_node, prev_out, key_lo);
                if (valid && !whole && mine.head_node >= 0) st.contig(mine.head_node, mine.head_len + (link ? prev_out : 0), key_lo);
                const int last = (n_chunks - c0 < 64 ? n_chunks - c0 : 64) - 1;
                carry_node = gs_readlane(mine.tail_node, last);
                carry_out = gs_readlane(val, last);
            }
            if (found && carry_node >= 0 && lane == 0) st.contig(carry_node, carry_out, key_lo);  // tail flush (:455-473)
        }
        if (found) {
            out_flags = GS_F_FOUND | GS_F_RETURNED;
            // ---- the distinct nodes in order of first appearance: reads1KMer and the candidate paths (two register sets: up to 128)
            int path[2] = {-1, -1}, ptin[2] = {0, 0}, ptout[2] = {0, 0}, used = 0;
            uint32_t last_pos = 0;
            for (int step = 0; step < n_touch; step++) {
                // the node with the smallest first position beyond the last one taken (one node per position: a tie is the same node twice)
                uint32_t best = 0xffffffffu;
                int best_v = -1;
                for (int i = lane; i < n_touch; i += 64) {
                    const int v = (int)touch[i];
                    const uint32_t fp = first[v];
                    if ((step == 0 || fp > last_pos) && fp < best) {
                        best = fp;
                        best_v = v;
                    }
                }
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const uint32_t ob = (uint32_t)__shfl_xor((int)best, o);
                    const int ov = __shfl_xor(best_v, o);
                    if (ob < best) {
                        best = ob;
                        best_v = ov;
                    }
                }
                best = (uint32_t)gs_rfl((int)best);
                const int nvj = gs_rfl(best_v);
                if (nvj < 0) break;
                last_pos = best;
                if (lane == 0) st.add(nvj, GS_S_READS_1KMER, 1);
                if (P.classify) {  // mergeReadTaxidPath (:568-586), as gs_process_read
                    const int ntin = st.tin[nvj], ntout = st.tout[nvj];
                    bool related = false;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        if (!related) {
                            const bool mine = 64 * h + lane < used;
                            const bool a = mine && gs_anc_or_self(ptin[h], ptout[h], ntin);
                            const bool b = mine && gs_anc_or_self(ntin, ntout, ptin[h]);
                            const u64 m = __ballot(a || b);
                            if (m) {
                                const int i = __builtin_ctzll(m);
                                if (lane == i && a) {
                                    path[h] = nvj;
                                    ptin[h] = ntin;
                                    ptout[h] = ntout;
                                }
                                related = true;
                            }
                        }
                    }
                    if (!related && used < P.max_paths) {
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            if (64 * h + lane == used) {
                                path[h] = nvj;
                                ptin[h] = ntin;
                                ptout[h] = ntout;
                            }
                        }
                        used++;
                    }
                }
            }
            // ---- classification (:474-531) from the vote counts, as the long-read path does it from its rows
            if (P.classify) {
                const double m = P.max_read_tax_err;
                const bool disabled = m >= 0 && ((m >= 1 && (double)tax_err > m) || ((double)tax_err > m * (double)max));
                if (!disabled) {
                    int cn = -1, first_node = -1, best = 0;
                    int sum[2] = {0, 0};
#pragma unroll
                    for (int h = 0; h < 2; h++)
                        if (64 * h + lane < used)
                            for (int x = path[h]; x >= 0; x = st.parent[x]) sum[h] += (int)cnt[x];
                    u64 tie_mask[2] = {0, 0};
                    for (int i = 0; i < used; i++) {
                        const int si = i < 64 ? gs_readlane(sum[0], i) : gs_readlane(sum[1], i - 64);
                        if (si > best) {
                            best = si;
                            tie_mask[0] = tie_mask[1] = 0;
                        }
                        if (si >= best) tie_mask[i >> 6] |= 1ULL << (i & 63);
                    }
                    int cand[2] = {path[0], path[1]};
                    if (P.threshold > 1) {  // lowestNodeWhereSumAboveThreshold per tied path (SmallTaxTree.java:208-221)
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            int mapped = -1;
                            if ((tie_mask[h] >> lane) & 1ULL) {
                                int acc = 0;
                                for (int x = path[h]; x >= 0 && mapped < 0; x = st.parent[x]) {
                                    const int cx = (int)cnt[x];
                                    if (cx != 0) {
                                        acc += cx;
                                        if (acc >= P.threshold) mapped = x;
                                    }
                                }
                            }
                            cand[h] = mapped;
                        }
                    }
                    {
                        bool firstc = true;
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            u64 tm = tie_mask[h];
                            while (tm) {
                                const int i = __builtin_ctzll(tm);
                                tm &= tm - 1;
                                const int x = gs_readlane(cand[h], i);
                                if (firstc) {
                                    cn = x;
                                    first_node = x;
                                    firstc = false;
                                } else
                                    cn = gs_lca(st, cn, x);
                            }
                        }
                    }
                    out_class = cn;
                    if (cn < 0) {
                        out_flags &= ~GS_F_RETURNED;
                    } else {
                        int read_kmers = best;
                        if (P.threshold > 1) {
                            read_kmers = 0;
                            for (int x = first_node; x >= 0; x = st.parent[x]) read_kmers += (int)cnt[x];
                        }
                        const int class_err = max - read_kmers;
                        const double mc = P.max_read_class_err;
                        if (mc < 0 || (mc >= 1 && (double)class_err <= mc) || ((double)class_err <= mc * (double)max)) {
                            out_flags |= GS_F_COUNTED;
                            if (lane == 0) {
                                const double err = (double)tax_err / (double)max;
                                const double cerr = (double)class_err / (double)max;
                                st.add(cn, GS_S_READS, 1);
                                st.add(cn, GS_S_READS_KMERS, (u64)read_kmers);
                                st.add(cn, GS_S_READS_BPS, (u64)L);
                                st.dadd(cn, GS_D_ERR_SUM, err);
                                st.dadd(cn, GS_D_ERR_SQ_SUM, err * err);
                                st.dadd(cn, GS_D_CLASS_ERR_SUM, cerr);
                                st.dadd(cn, GS_D_CLASS_ERR_SQ_SUM, cerr * cerr);
                            }
                        }
                    }
                }
            }
        }
        if (lane == 0) {
            if (P.class_vi) P.class_vi[r] = out_class;
            if (P.flags) P.flags[r] = (uint8_t)out_flags;
        }
        // the read's rows, clean for the next batch (every lane has read what it needs of them: the writes come last)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < n_touch; i += 64) {
            const int v = (int)touch[i];
            cnt[v] = 0;
            for (int cp = 0; cp < GS_HUGE_COPIES; cp++) {
                cnt_c[(size_t)cp * nv + v] = 0;
                first_c[(size_t)cp * nv + v] = 0xffffffffu;
            }
        }
        if (lane < GS_HUGE_COPIES) hd[lane].n_miss = hd[lane].bad_lo = hd[lane].flags = hd[lane].n_touch = 0;
    }
    GS_STATS_EPILOGUE()
}

// ---------------------------------------------------------------------------------------------------
// the deferred statistics (GsStatRec) of a batch into the counters: one LDS table per workgroup for the value indices
// [lo, hi) -- this kernel has the whole LDS for it --, flushed with one global atomic per touched counter and workgroup
// ---------------------------------------------------------------------------------------------------
#define GS_REDUCE_VALUES 640
// the value indices of the records as an array of their own: with more than 640 values the reduce runs once per 640 of them, and a
// pass that reads 4 bytes per record instead of touching every 64-byte record is 16 times lighter
__global__ __launch_bounds__(256) void gs_stat_vi_kernel(const GsStatRec *recs, const u64 *count, int32_t *vi) {
    const int64_t n = (int64_t)*count;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) vi[i] = recs[i].vi;
}

__global__ __launch_bounds__(1024) void gs_stat_reduce_kernel(const GsStatRec *recs, const int32_t *vis, const u64 *count, int lo, int hi, u64 *sums,
                                                              u64 *maxk, double *dsums) {
    const int64_t n = (int64_t)*count;  // (0 for a refused text chunk: the match kernel handed out no records)
    if (n == 0) return;
    __shared__ u64 s_sums[GS_REDUCE_VALUES * GS_N_SUMS];
    __shared__ u64 s_max[GS_REDUCE_VALUES];
    __shared__ double s_d[GS_REDUCE_VALUES * GS_N_DCOLS];
    const int nvl = hi - lo;
    for (int i = threadIdx.x; i < nvl * GS_N_SUMS; i += blockDim.x) s_sums[i] = 0;
    for (int i = threadIdx.x; i < nvl; i += blockDim.x) s_max[i] = 0;
    for (int i = threadIdx.x; i < nvl * GS_N_DCOLS; i += blockDim.x) s_d[i] = 0.0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int vi = vis ? vis[i] : recs[i].vi;
        if (vi < lo || vi >= hi) continue;
        const GsStatRec rc = recs[i];
        u64 *row = s_sums + (size_t)(vi - lo) * GS_N_SUMS;
        atomicAdd(&row[GS_S_READS_1KMER], 1ULL);
        atomicAdd(&row[GS_S_KMERS], (u64)rc.kmers);
        atomicAdd(&row[GS_S_CONTIGS], (u64)rc.contigs);
        atomicAdd(&row[GS_S_CONTIG_LEN_SQ_SUM], (u64)rc.sq);
        atomicMax(&s_max[vi - lo], rc.max_key);
        if (rc.counted) {
            double *dr = s_d + (size_t)(vi - lo) * GS_N_DCOLS;
            atomicAdd(&row[GS_S_READS], 1ULL);
            atomicAdd(&row[GS_S_READS_KMERS], (u64)rc.read_kmers);
            atomicAdd(&row[GS_S_READS_BPS], (u64)rc.read_len);
            // (formed here, one thread per record, and not by lane 0 of the wave that wrote it)
            const double err = (double)rc.tax_err / (double)rc.n_pos;
            const double cerr = (double)(rc.n_pos - rc.read_kmers) / (double)rc.n_pos;
            atomicAdd(&dr[GS_D_ERR_SUM], err);
            atomicAdd(&dr[GS_D_ERR_SQ_SUM], err * err);
            atomicAdd(&dr[GS_D_CLASS_ERR_SUM], cerr);
            atomicAdd(&dr[GS_D_CLASS_ERR_SQ_SUM], cerr * cerr);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nvl * GS_N_SUMS; i += blockDim.x)
        if (s_sums[i]) atomicAdd(&sums[(size_t)lo * GS_N_SUMS + i], s_sums[i]);
    for (int i = threadIdx.x; i < nvl; i += blockDim.x)
        if (s_max[i]) atomicMax(&maxk[lo + i], s_max[i]);
    for (int i = threadIdx.x; i < nvl * GS_N_DCOLS; i += blockDim.x)
        if (s_d[i] != 0.0) atomicAdd(&dsums[(size_t)lo * GS_N_DCOLS + i], s_d[i]);
}

// n_values <= GS_STAT_REC_MAX_VALUES: a pass of gs_stat_reduce_kernel per 640 values
// n_max: upper bound of the record count (the kernels read the real one from *count)
// vi_scratch: room for n_max value indices, used when the reduce takes more than one pass (nullptr: every pass reads the records)
extern "C" hipError_t gs_launch_stat_reduce(const GsStatRec *recs, const void *count, int64_t n_max, int n_values, void *sums, void *maxk,
                                             void *dsums, int32_t *vi_scratch, hipStream_t stream) {
    if (n_max <= 0) return hipSuccess;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n_max + 8191) / 8192, 512));
    const int32_t *vis = nullptr;
    if (vi_scratch != nullptr && n_values > GS_REDUCE_VALUES) {
        hipLaunchKernelGGL(gs_stat_vi_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n_max + 1023) / 1024, 4096))), dim3(256), 0, stream,
                           recs, (const u64 *)count, vi_scratch);
        vis = vi_scratch;
    }
    for (int lo = 0; lo < n_values; lo += GS_REDUCE_VALUES)
        hipLaunchKernelGGL(gs_stat_reduce_kernel, dim3(grid), dim3(1024), 0, stream, recs, vis, (const u64 *)count, lo,
                           std::min(n_values, lo + GS_REDUCE_VALUES), (u64 *)sums, (u64 *)maxk, (double *)dsums);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// launchers (called from gs_api.cpp)
// ---------------------------------------------------------------------------------------------------
static size_t gs_stats_lds_bytes(int n_values) {
    if (n_values <= GS_NV_LDS) return (size_t)n_values * ((GS_N_SUMS + 1 + GS_N_DCOLS) * 8 + 3 * 4);
    return n_values <= GS_NV_TREE_LDS ? (size_t)n_values * 3 * 4 : 0;  // the tree alone
}

// GS_FORCE_GLOBAL_STATS=1 (developer knob): the kernels for stores with more values than the LDS counters hold, on any store.
// Read ONCE per process here (a static) but on every run by gs_match_begin (gs_api.cpp), which sizes the counters by it: set or
// cleared after the first launch, the two disagree -- never change it inside a process (the tests reach these kernels through
// real value counts instead)
static bool gs_force_global_stats() {
    static const bool on = [] {
        const char *e = getenv("GS_FORCE_GLOBAL_STATS");
        return e != nullptr && atoi(e) != 0;
    }();
    return on;
}

template <bool FROM_NODES, int KC, bool WIDE, bool STRIPED, int CTX>
static void gs_launch_match_t(const GsMatchParams *P, int grid, size_t lds, bool lds_stats, hipStream_t stream) {
    if (lds_stats)
        hipLaunchKernelGGL((gs_match_kernel<true, FROM_NODES, KC, WIDE, STRIPED, CTX>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P);
    else
        hipLaunchKernelGGL((gs_match_kernel<false, FROM_NODES, KC, WIDE, STRIPED, CTX>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P);
}

// k = 31 (the reference's default and maximum) runs kernels with k folded in at compile time; whether the gate is keyed by
// minimizer + context (big stores, GsDbDev::mgate_ctx) is folded in as well -- the branch alone costs the common kernels 3 % --
// except in the 128-path variants, which ask the store
extern "C" hipError_t gs_launch_match(const GsMatchParams *P, int grid, hipStream_t stream) {
    const size_t lds = gs_stats_lds_bytes(P->db.n_values);
    const bool lds_stats = P->db.n_values <= GS_NV_LDS && !gs_force_global_stats();
    const bool ctx = P->db.mgate_ctx != 0;
    // (a row of P.sn_nodes holds node codes in 16 bits: value indices below 2^15 next to the negative codes)
    if (P->sn_nodes != nullptr && (!lds_stats || P->db.n_values > GS_SN_CODE_MAX)) return hipErrorInvalidValue;
    // (the gate-less loop is the FIXED loop of the one-store, 64-path kernels whose gate is keyed by the minimizer alone, on a store
    // with a gate and records: anywhere else the flag would be ignored in silence)
    if (P->fixed_nogate != 0 &&
        (P->db.n_parts > 1 || P->nodes != nullptr || P->max_paths > 64 || ctx || P->db.mgate == nullptr || P->db.rec == nullptr ||
         P->off_stride != 0 || P->quot == nullptr || P->fixed_len < 128 || P->fixed_len - P->db.k + 1 > 128 ||
         (lds_stats && (P->sn_recs == nullptr || P->sn_nodes == nullptr))))
        return hipErrorInvalidValue;
    if (P->db.n_parts > 1) {  // striped store (always probed locally: nodes == nullptr)
        if (P->nodes != nullptr) return hipErrorInvalidValue;
        if (P->max_paths > 64)
            gs_launch_match_t<false, 0, true, true, 2>(P, grid, lds, lds_stats, stream);
        else if (P->db.k == 31)
            ctx ? gs_launch_match_t<false, 31, false, true, 1>(P, grid, lds, lds_stats, stream)
                : gs_launch_match_t<false, 31, false, true, 0>(P, grid, lds, lds_stats, stream);
        else
            ctx ? gs_launch_match_t<false, 0, false, true, 1>(P, grid, lds, lds_stats, stream)
                : gs_launch_match_t<false, 0, false, true, 0>(P, grid, lds, lds_stats, stream);
        return hipGetLastError();
    }
    if (P->nodes != nullptr) {  // DB-partitioned mode: the nodes come from the owners, nothing is probed here
        if (P->max_paths > 64)
            gs_launch_match_t<true, 0, true, false, 0>(P, grid, lds, lds_stats, stream);
        else
            gs_launch_match_t<true, 0, false, false, 0>(P, grid, lds, lds_stats, stream);
        return hipGetLastError();
    }
    if (P->max_paths > 64)  // two candidate paths per lane (the reference allows up to 128, C/GSConfigKey.java:350)
        gs_launch_match_t<false, 0, true, false, 2>(P, grid, lds, lds_stats, stream);
    else if (P->db.k == 31)
        ctx ? gs_launch_match_t<false, 31, false, false, 1>(P, grid, lds, lds_stats, stream)
            : gs_launch_match_t<false, 31, false, false, 0>(P, grid, lds, lds_stats, stream);
    else
        ctx ? gs_launch_match_t<false, 0, false, false, 1>(P, grid, lds, lds_stats, stream)
            : gs_launch_match_t<false, 0, false, false, 0>(P, grid, lds, lds_stats, stream);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_match_long(const GsMatchParams *P, int grid, int32_t *scratch, uint32_t *serial,
                                           hipStream_t stream) {
    const size_t lds = gs_stats_lds_bytes(P->db.n_values);
    const bool lds_stats = P->db.n_values <= GS_NV_LDS && !gs_force_global_stats();
    if (P->db.n_parts > 1) {
        if (P->nodes != nullptr) return hipErrorInvalidValue;
        if (P->max_paths > 64) {
            if (lds_stats)
                hipLaunchKernelGGL((gs_match_long_kernel<true, false, true, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
            else
                hipLaunchKernelGGL((gs_match_long_kernel<false, false, true, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
        } else {
            if (lds_stats)
                hipLaunchKernelGGL((gs_match_long_kernel<true, false, false, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
            else
                hipLaunchKernelGGL((gs_match_long_kernel<false, false, false, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
        }
        return hipGetLastError();
    }
    if (P->max_paths > 64) {
        if (P->nodes == nullptr) {
            if (lds_stats)
                hipLaunchKernelGGL((gs_match_long_kernel<true, false, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
            else
                hipLaunchKernelGGL((gs_match_long_kernel<false, false, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
        } else {
            if (lds_stats)
                hipLaunchKernelGGL((gs_match_long_kernel<true, true, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
            else
                hipLaunchKernelGGL((gs_match_long_kernel<false, true, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
        }
        return hipGetLastError();
    }
    if (P->nodes == nullptr) {
        if (P->db.k == 31) {  // (as gs_match_kernel: k folded in at compile time)
            if (lds_stats)
                hipLaunchKernelGGL((gs_match_long_kernel<true, false, false, false, 31>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
            else
                hipLaunchKernelGGL((gs_match_long_kernel<false, false, false, false, 31>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
        } else if (lds_stats)
            hipLaunchKernelGGL((gs_match_long_kernel<true, false>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
        else
            hipLaunchKernelGGL((gs_match_long_kernel<false, false>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
    } else {
        if (lds_stats)
            hipLaunchKernelGGL((gs_match_long_kernel<true, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
        else
            hipLaunchKernelGGL((gs_match_long_kernel<false, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P, scratch, serial);
    }
    return hipGetLastError();
}

// the copies 1 .. copies - 1 of the run's counters into copy 0 (sums and double sums added, max keys by maximum), the copies zeroed:
// one launch (one per copy and array -- 45 for 16 copies -- cost 0.2 ms per job).  GS_FOLD_LANES lanes per cell, each with every
// GS_FOLD_LANES-th copy, so that the loads of a cell's copies are in flight together (one thread per cell walked them as one
// dependent chain: 12.7 us for 140 cells x 16 copies).  `result`, when given, receives the totals in the layout of
// gs_match_finish's landing area (sums | max keys | unique counts | double sums) with the unique counts zeroed.
#define GS_FOLD_LANES 16
template <typename T, bool MAX>
static __device__ __forceinline__ T gs_fold_cell(T *a, long long n, long long i, int copies, int j) {
    T acc = 0;
    for (int c = j; c < copies; c += GS_FOLD_LANES) {
        const T x = a[(long long)c * n + i];
        acc = MAX ? (x > acc ? x : acc) : acc + x;
        if (c != 0) a[(long long)c * n + i] = 0;
    }
#pragma unroll
    for (int d = GS_FOLD_LANES / 2; d >= 1; d >>= 1) {
        const T x = __shfl_xor(acc, d, GS_FOLD_LANES);
        acc = MAX ? (x > acc ? x : acc) : acc + x;
    }
    if (j == 0) a[i] = acc;
    return acc;
}
__global__ __launch_bounds__(256) void gs_fold_stats_kernel(long long *sums, unsigned long long *maxk, double *dsums, long long nv, int copies,
                                                           unsigned long long *result) {
    const int j = (int)(threadIdx.x % GS_FOLD_LANES);
    long long i = ((long long)blockIdx.x * 256 + threadIdx.x) / GS_FOLD_LANES;  // the cell: sums, then max keys, then double sums
    const long long n_s = nv * GS_N_SUMS, n_d = nv * GS_N_DCOLS;
    if (i < n_s) {
        const long long a = gs_fold_cell<long long, false>(sums, n_s, i, copies, j);
        if (result && j == 0) result[i] = (unsigned long long)a;
        return;
    }
    i -= n_s;
    if (i < nv) {
        const unsigned long long m = gs_fold_cell<unsigned long long, true>(maxk, nv, i, copies, j);
        if (result && j == 0) result[n_s + i] = m;
        if (result && j == 1) result[n_s + nv + i] = 0;
        return;
    }
    i -= nv;
    if (i < n_d) {
        const double a = gs_fold_cell<double, false>(dsums, n_d, i, copies, j);
        if (result && j == 0) reinterpret_cast<double *>(result)[n_s + 2 * nv + i] = a;
    }
}
extern "C" hipError_t gs_launch_fold_stats(long long *sums, unsigned long long *maxk, double *dsums, long long nv, int copies,
                                           unsigned long long *result, hipStream_t stream) {
    const long long n = nv * (GS_N_SUMS + 1 + GS_N_DCOLS) * GS_FOLD_LANES;
    hipLaunchKernelGGL(gs_fold_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sums, maxk, dsums, nv, copies, result);
    return hipGetLastError();
}

// which of the wide kernels (bit 0: three sub-rounds, reads of 129 .. 192 positions; bit 1: four, 193 .. 256) serve this store and run
extern "C" int gs_match_wide_mask(const GsMatchParams *P) {
    if (P->nodes != nullptr || P->db.n_parts > 1 || P->max_paths > 64) return 0;
    return 3;
}
// ns = 3 / 4: the reads of that queue -- or all reads of the batch when P->long_list is null -- each in one trip; grid: the device's CUs
extern "C" hipError_t gs_launch_match_wide(const GsMatchParams *P, int ns, int n_cu, hipStream_t stream) {
    if ((ns != 3 && ns != 4) || ((gs_match_wide_mask(P) >> (ns - 3)) & 1) == 0) return hipErrorNotSupported;
    const size_t lds = gs_stats_lds_bytes(P->db.n_values);
    const bool lds_stats = P->db.n_values <= GS_NV_LDS && !gs_force_global_stats();
    const int v = (lds_stats ? 4 : 0) | (ns == 4 ? 2 : 0) | (P->db.k == 31 ? 1 : 0);
    void (*kern)(GsMatchParams) = nullptr;
    switch (v) {
        case 0: kern = gs_match_wide_kernel<false, 3, 0>; break;
        case 1: kern = gs_match_wide_kernel<false, 3, 31>; break;
        case 2: kern = gs_match_wide_kernel<false, 4, 0>; break;
        case 3: kern = gs_match_wide_kernel<false, 4, 31>; break;
        case 4: kern = gs_match_wide_kernel<true, 3, 0>; break;
        case 5: kern = gs_match_wide_kernel<true, 3, 31>; break;
        case 6: kern = gs_match_wide_kernel<true, 4, 0>; break;
        default: kern = gs_match_wide_kernel<true, 4, 31>; break;
    }
    static int occ_of[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // resident workgroups per CU (dynamic LDS aside: small against the static part)
    int occ = occ_of[v];
    if (occ == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, GS_BLOCK, lds) != hipSuccess || occ < 1) occ = 1;
        occ_of[v] = occ;
    }
    hipLaunchKernelGGL(kern, dim3(n_cu * occ), dim3(GS_BLOCK), lds, stream, *P);
    return hipGetLastError();
}

// reads of GS_HUGE_MIN positions and more that the match kernel handed over: chunks over the whole device, then one wave per read
extern "C" hipError_t gs_launch_match_huge(const GsMatchParams *P, int grid, hipStream_t stream) {
    if (P->huge_count == nullptr || P->nodes != nullptr) return hipSuccess;
    const size_t lds = gs_stats_lds_bytes(P->db.n_values);
    const bool lds_stats = P->db.n_values <= GS_NV_LDS && !gs_force_global_stats();
    const bool striped = P->db.n_parts > 1;
    if (lds_stats) {
        if (striped)
            hipLaunchKernelGGL((gs_match_huge_kernel<true, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P);
        else if (P->db.k == 31)
            hipLaunchKernelGGL((gs_match_huge_kernel<true, false, 31>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P);
        else
            hipLaunchKernelGGL((gs_match_huge_kernel<true, false>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P);
        hipLaunchKernelGGL((gs_match_huge_finish_kernel<true>), dim3(GS_HUGE_SLOTS / (GS_BLOCK / 64)), dim3(GS_BLOCK), lds, stream, *P);
    } else {
        if (striped)
            hipLaunchKernelGGL((gs_match_huge_kernel<false, true>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P);
        else if (P->db.k == 31)
            hipLaunchKernelGGL((gs_match_huge_kernel<false, false, 31>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P);
        else
            hipLaunchKernelGGL((gs_match_huge_kernel<false, false>), dim3(grid), dim3(GS_BLOCK), lds, stream, *P);
        hipLaunchKernelGGL((gs_match_huge_finish_kernel<false>), dim3(GS_HUGE_SLOTS / (GS_BLOCK / 64)), dim3(GS_BLOCK), lds, stream, *P);
    }
    return hipGetLastError();
}

extern "C" int gs_match_occupancy(int n_values) {
    int n = 0;
    hipError_t e = n_values <= GS_NV_LDS
                       ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gs_match_kernel<true, false, 31>, GS_BLOCK, gs_stats_lds_bytes(n_values))
                       : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gs_match_kernel<false, false, 31>, GS_BLOCK, gs_stats_lds_bytes(n_values));
    return e == hipSuccess ? n : 0;
}

// workgroups of the long-read kernel a CU holds at once (the plain variant stands for all of them)
extern "C" int gs_match_long_occupancy(int n_values) {
    int n = 0;
    hipError_t e = n_values <= GS_NV_LDS
                       ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gs_match_long_kernel<true, false, true, true>, GS_BLOCK, gs_stats_lds_bytes(n_values))
                       : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, gs_match_long_kernel<false, false, true, true>, GS_BLOCK, gs_stats_lds_bytes(n_values));
    return e == hipSuccess ? n : 0;
}
