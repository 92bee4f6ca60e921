// gs_wave.h -- device code that more than one kernel family shares: lane helpers, bases -> ballot planes, the store probe of 128
// k-mer positions of one read on one wave (gs_probe_planes) and what it is built from.  Included by gs_kernels.hip (match),
// gs_route.hip, gs_segments.hip, gs_seen.hip and gs_filter.hip; a helper with one family of users lives in that family's unit.
// The match kernels are sensitive to the very text of what they inline ("Source layout"): text that moves into or
// out of this header is checked against the parent commit's device assembly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_layout.h"
#include "gs_params.h"

// developer ablations (tools/ablate.sh): 1 = no per-read reduce, 2 = no record / table probe, 4 = no gate either,
// 8 = no statistics atomics
#ifndef GS_ABLATE
#define GS_ABLATE 0
#endif

#define GS_NODE_MISS (-1)
#define GS_NODE_INVALID (-2)
#define GS_NODE_NONE (-3)

__device__ __forceinline__ int gs_lane() { return (int)__lane_id(); }
__device__ __forceinline__ int gs_readlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int gs_rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
// x without bit `bit`, both wave-uniform: one scalar instruction where `x &= x - 1` is three
__device__ __forceinline__ unsigned long long gs_bitset0(unsigned long long x, int bit) {
    asm("s_bitset0_b64 %0, %1" : "+s"(x) : "s"(bit));
    return x;
}
// `old` with lane LANE replaced by the wave-uniform v (v_writelane_b32: scalar source, no exec region, no select)
template <int LANE>
__device__ __forceinline__ int gs_writelane(int old, int v) {
    asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(v), "n"(LANE));
    return old;
}

// developer instrumentation (tools/phase_times.sh: -DGS_PHASE=1): wave cycles per phase of the short-read path, summed over all
// waves (s_memtime at the phase boundaries; `dep` is a value the phase produces, so the stamp sits behind the wait for it)
#ifndef GS_PHASE
#define GS_PHASE 0
#endif
#if GS_PHASE
// (internal linkage: every unit that includes this header times into a copy of its own; gs_debug_phase, gs_kernels.hip, reads the
// match unit's -- only match kernels flush their stamps)
static __device__ unsigned long long gs_phase_acc[16];
__device__ __forceinline__ unsigned long long *gs_phase_row() {
    __shared__ unsigned long long ph[4][16];
    return ph[threadIdx.x >> 6];
}
__device__ __forceinline__ void gs_stamp(int i) {
    const unsigned long long t = __builtin_readcyclecounter();
    if (gs_lane() == 0) {
        unsigned long long *p = gs_phase_row();
        const unsigned long long last = p[15];
        p[15] = t;
        if (i >= 0) p[i] += t - last;
    }
}
#define GS_STAMP(i, dep)                \
    {                                   \
        asm volatile("" ::"v"(dep));    \
        gs_stamp(i);                    \
    }
#else
#define GS_STAMP(i, dep) {}
#endif

// bits [s, s+64) of the 128-bit string (b:a), s in 0..63
__device__ __forceinline__ u64 gs_funnel(u64 a, u64 b, int s) { return (a >> s) | ((b << 1) << (63 - s)); }

// ASCII bases -> ballot planes of the reference's 2-bit codes (C0 G1 A2 T3, upper case only: CGAT.java:66-69), from a byte that was
// loaded earlier; lanes beyond the read hold GS_FILL ('C': code 0, valid -- planes 0 and not bad, without a range test).
// Straight-line, every ballot one integer compare: x = bits 1..2 of the byte (A 0, C 1, T 2, G 3), d = byte ^ the one upper-case
// letter with that x (a byte permute), code-hi = x even, code-lo = bit 2 of the byte; a byte that is not its letter (N, lower
// case, CR, NUL) has d != 0: planes 0 -- every window that holds such a byte is INVALID whatever its planes say -- and bad.
#define GS_FILL 0x43u
__device__ __forceinline__ void gs_word_from_byte(uint32_t c, u64 &hi, u64 &lo, u64 &bad) {
    const uint32_t x = (c >> 1) & 3u;
    const uint32_t d = c ^ __builtin_amdgcn_perm(0u, 0x47544341u, x | 0x0c0c0c00u);
    hi = __ballot(((x & 1u) | d) == 0u);
    lo = __ballot((((c ^ 4u) & 4u) | d) == 0u);
    bad = __ballot(d != 0u);
}
// The same for the FIXED loop of gs_match_kernel, without the forced zero: the planes of a byte that is not its letter are whatever
// its bits 1 and 2 say (four vector instructions fewer per word).  A letter and the fill byte get the planes they get above: hi =
// "x even" is bit 1 clear, lo is bit 2, and GS_FILL has bit 1 set and bit 2 clear.  Nobody can tell the planes of a bad byte b:
//  - a window that holds b is INVALID by `bad` alone (gs_probe_planes: the funnel over Bbad), and the census counts `bad` alone;
//  - ranks: the k-mer at position p reads the ranks of the 15-mers at p .. p + k - 15, whose bases are p .. p + k - 1, its own.  A
//    15-mer that holds b is read by windows that hold b only, all of them INVALID.  A rank carries its row index in its low eight
//    bits whatever the hash was, so the index a dead lane takes from a wrong minimum is still one of the row's 144;
//  - the 15-mer read back (cf) is the one at the chosen index: inside a valid window's own bases, anything in a dead lane, where
//    the gate key, the oriented planes and the record offset made from it are computed and never used: a dead lane reads gate word 0
//    (the address select is by `act`), and the record loads, the table walk and every mark sit behind `act`;
//  - the tail round (positions 128 .. 143) reads word 2 alone: its lanes beyond the read hold GS_FILL, planes 0 as before, and a
//    bad byte there is again seen by windows that hold it only.
__device__ __forceinline__ void gs_word_from_byte_fixed(uint32_t c, u64 &hi, u64 &lo, u64 &bad) {
    const uint32_t x = (c >> 1) & 3u;
    const uint32_t d = c ^ __builtin_amdgcn_perm(0u, 0x47544341u, x | 0x0c0c0c00u);
    hi = __ballot((c & 2u) == 0u);
    lo = __ballot((c & 4u) != 0u);
    bad = __ballot(d != 0u);
}

// one 64-base word of a read -> ballot planes
__device__ __forceinline__ void gs_load_word(const uint8_t *rd, int L, int w, int lane, u64 &hi, u64 &lo, u64 &bad) {
    const int j = 64 * w + lane;
    const uint32_t c = j < L ? rd[j] : GS_FILL;
    gs_word_from_byte(c, hi, lo, bad);
}

// ---------------------------------------------------------------------------------------------------
// store probe
// ---------------------------------------------------------------------------------------------------
typedef unsigned long long gs_u64x2 __attribute__((ext_vector_type(2)));

// The fused kernels look at the first half of a bucket first (two loads, four compares, half the registers) and run
// at 8 waves per SIMD with 64 VGPRs.  Measured against whole-bucket probes at 6 waves: bench stream equal (10.26 ms),
// miss-only stream 5.94 -> 5.56 ms, 47 M-k-mer store 16.3 -> 16.0 ms.
#ifndef GS_HALF_BUCKETS
#define GS_HALF_BUCKETS 1
#endif
#ifndef GS_WAVES
#define GS_WAVES 8
#endif

// (Software pipelining across the reads of a wave -- offsets two reads ahead, bases one read ahead -- was measured on
// MI355X in round 1 and again in round 2 on the record layout, also on the HBM-resident 47 M-k-mer store: within noise
// (7.67 / 7.79 ms, 10.45 / 10.53 ms) while costing 4 more spilled VGPRs; the code is gone.)

#ifndef GS_NT_TABLE
// Measured on MI355X: non-temporal bucket loads stop the four dwordx4 loads of one 64-byte line from sharing a
// single L2 request (the match kernel ran 2.2x slower), so the default is plain loads.
#define GS_NT_TABLE 0
#endif

struct GsBucket {
    gs_u64x2 q[4];
};

__device__ __forceinline__ void gs_load_bucket(const u64 *table, u64 bkt, GsBucket &b) {
    const gs_u64x2 *p = reinterpret_cast<const gs_u64x2 *>(table + bkt * GS_SLOTS_PER_BUCKET);
#if GS_NT_TABLE
    b.q[0] = __builtin_nontemporal_load(p);
    b.q[1] = __builtin_nontemporal_load(p + 1);
    b.q[2] = __builtin_nontemporal_load(p + 2);
    b.q[3] = __builtin_nontemporal_load(p + 3);
#else
    b.q[0] = p[0];
    b.q[1] = p[1];
    b.q[2] = p[2];
    b.q[3] = p[3];
#endif
}

// returns true when the probe is finished (hit, or miss proven by a non-full bucket).
// slot = rem << (vbits+3) | disp << (vbits+1) | (vi+1) << 1 | seen, with vbits+3 < 32: a match has an equal high
// dword and a low dword that differs from `want` (value and seen fields 0) by x = 2(vi+1) + seen, i.e.
// 0 <= x-2 < 2*vmask.  On a hit vs = 2*vi + seen.  Buckets fill front to back, so "full" is "slot 7 is occupied".
__device__ __forceinline__ bool gs_match_bucket(const GsBucket &b, u64 want, uint32_t vmask2, int &vs, int &slot) {
    const u64 s[8] = {b.q[0].x, b.q[0].y, b.q[1].x, b.q[1].y, b.q[2].x, b.q[2].y, b.q[3].x, b.q[3].y};
    // two instructions per slot: mask the value/seen field away and compare all 64 bits.  An empty slot (0) can only
    // "match" want == 0 and is told apart afterwards by its zero value field.
    const u64 keep = ~(u64)(vmask2 + 1u);  // vmask2 + 1 = 2^(vbits+1) - 1: the (vi+1, seen) field
    int hit = -1;
    uint32_t low = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--) {  // buckets fill front to back: the lowest match is the real entry
        const bool m = (s[j] & keep) == want;
        low = m ? (uint32_t)s[j] : low;
        hit = m ? j : hit;
    }
    const int x = (int)(low & (vmask2 + 1u)) - 2;  // 2 vi + seen, or < 0 for the empty slot
    if (hit >= 0 && x >= 0) {
        vs = x;
        slot = hit;
        return true;
    }
    return s[7] == 0;
}

// Half a bucket (slots 0-3 or 4-7, 32 bytes).  Buckets fill front to back and hold 1.5 .. 3 keys on average, so the
// first half answers most probes with two load instructions, four slot compares and half the registers.
struct GsHalf {
    gs_u64x2 q[2];
};

__device__ __forceinline__ void gs_load_half(const u64 *table, u64 bkt, int half, GsHalf &b) {
    const gs_u64x2 *p = reinterpret_cast<const gs_u64x2 *>(table + bkt * GS_SLOTS_PER_BUCKET) + 2 * half;
    b.q[0] = p[0];
    b.q[1] = p[1];
}

// as gs_match_bucket over four slots; finished = hit, or the half's last slot is empty (nothing can follow it)
__device__ __forceinline__ bool gs_match_half(const GsHalf &b, u64 want, uint32_t vmask2, int &vs, int &slot) {
    const u64 s[4] = {b.q[0].x, b.q[0].y, b.q[1].x, b.q[1].y};
    const u64 keep = ~(u64)(vmask2 + 1u);
    int hit = -1;
    uint32_t low = 0;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        const bool m = (s[j] & keep) == want;
        low = m ? (uint32_t)s[j] : low;
        hit = m ? j : hit;
    }
    const int x = (int)(low & (vmask2 + 1u)) - 2;
    if (hit >= 0 && x >= 0) {
        vs = x;
        slot = hit;
        return true;
    }
    return s[3] == 0;
}

// table hash of the k-mer whose forward planes are (fhi, flo): representative orientation, then the Feistel mix
__device__ __forceinline__ u64 gs_kmer_hash(uint32_t fhi, uint32_t flo, int k, uint32_t kmask) {
    uint32_t a, b;
    gs_rep_planes(fhi, flo, k, kmask, a, b);
    return gs_mix_planes(a, b);
}

// ---------------------------------------------------------------------------------------------------
// 128 k-mer positions [base, base+128) of one read: planes -> minimizer -> gate -> record line (or bucket line) -> node.
// node[s] for position base + 64 s + lane: value index (hit), GS_NODE_MISS, GS_NODE_INVALID (window holds a
// non-CGAT byte) or GS_NODE_NONE (position >= max).  Hits are marked on the spot (mk): the unique-k-mer "seen" bit of
// the slot / record offset that was just read (KMerUniqueCounterBits.putInlined; a k-mer that is already marked costs
// nothing, a stale copy only repeats the atomic) and the per-k-mer hit counter (maxKMerResCounts > 0).
// ---------------------------------------------------------------------------------------------------
struct GsMark {
    int count_unique;
    uint32_t *hit_counts;  // [table slots | GS_REC_SLOTS per record bucket] or nullptr
    // striped store: the store's memory is read-only (foreign stripes belong to other GPUs); the seen bits are this run's
    uint32_t *tab_seen;    // one bit per table slot
    uint32_t *rec_seen;    // one word per record bucket
};

// where a striped store keeps the pointers of its stripes: behind the two hash rows of the wave's LDS block
// (GS_STRIPE_TABLE): GS_MAX_STRIPES record stripes, then GS_MAX_STRIPES table stripes, all biased (gs_layout.h)
#define GS_ROW 160  // one LDS row: 128 + 16 positions, padded
#define GS_STRIPE_WORDS (4 * GS_MAX_STRIPES)
__device__ __forceinline__ const u64 *gs_rec_stripe(const GsDbDev &db, const uint32_t *wave_g, uint32_t bucket) {
    return reinterpret_cast<const u64 *const *>(wave_g + 2 * GS_ROW)[(bucket * db.n_parts) >> db.rec_bits];
}
__device__ __forceinline__ const u64 *gs_tab_stripe(const GsDbDev &db, const uint32_t *wave_g, uint32_t bucket) {
    return reinterpret_cast<const u64 *const *>(wave_g + 2 * GS_ROW)[GS_MAX_STRIPES + (((bucket >> 2) * db.n_parts) >> (db.bucket_bits - 2))];
}

template <bool STRIPED>
__device__ __forceinline__ void gs_take_hit(const GsDbDev &db, uint32_t slot, int vs, int &node, const GsMark &mk) {
    node = vs >> 1;
    if (STRIPED) {
        if (mk.count_unique) {
            uint32_t *w = mk.tab_seen + (slot >> 5);
            const uint32_t bit = 1u << (slot & 31);
            if ((*w & bit) == 0) atomicOr(w, bit);
        }
    } else if (mk.count_unique && (vs & 1) == 0)
        atomicOr(const_cast<u64 *>(db.table) + slot, 1ULL);
    if (mk.hit_counts != nullptr) atomicAdd(mk.hit_counts + slot, 1u);
}

// the rest of a table lookup for the lanes in `pending` (their k-mer was not decided by the first half of its home
// bucket, or that half has not been looked at yet: FIRST): second half, then the displaced buckets
template <bool FIRST, bool STRIPED>
__device__ __forceinline__ void gs_lookup_rest(const GsDbDev &db, uint32_t bkt, u64 want, uint32_t vmask2, bool pending, int &node,
                                               const GsMark &mk, const uint32_t *wave_g) {
    const uint32_t bmask = (uint32_t)db.bucket_mask;
#pragma unroll
    for (int half = FIRST ? 0 : 1; half < 2; half++) {
        if (__ballot(pending) != 0) {  // (second half: more than four entries in the home bucket)
            if (pending) {
                GsHalf t;
                gs_load_half(STRIPED ? gs_tab_stripe(db, wave_g, bkt) : db.table, bkt, half, t);
                int vs = -1, sl = 0;
                const bool done = gs_match_half(t, want, vmask2, vs, sl);
                if (vs >= 0) gs_take_hit<STRIPED>(db, bkt * GS_SLOTS_PER_BUCKET + 4 * half + sl, vs, node, mk);
                pending = !done;
            }
        }
    }
    // rare: home bucket full without a match -> walk the displaced buckets
    for (int disp = 1; disp <= GS_MAX_DISP && __ballot(pending) != 0; disp++) {
        if (pending) {
            const uint32_t b2 = (bkt + (uint32_t)disp) & bmask;
            GsBucket t;
            gs_load_bucket(STRIPED ? gs_tab_stripe(db, wave_g, b2) : db.table, b2, t);
            int vs = -1, sl = 0;
            const bool done = gs_match_bucket(t, want | ((u64)disp << (db.vbits + 1)), vmask2, vs, sl);
            if (vs >= 0) gs_take_hit<STRIPED>(db, b2 * GS_SLOTS_PER_BUCKET + sl, vs, node, mk);
            pending = !done;
        }
    }
}

// minimizer of the k-mers at positions base + 64 s + lane through the wave's LDS row: rank of every 15-mer of
// positions base .. base+143, then per lane the minimum over its k-14 positions (one min3 chain; the rank carries the
// row index, so the minimum is the position as well).  Returns the offset of the chosen 15-mer inside the lane's k-mer.
// wave_g: two rows of GS_ROW words per wave -- the ranks, and behind them (canonical 15-mer << 1 | strand) of every position,
// which the lane that picks a position reads back instead of recomputing it.  cf[s] = that word for the lane's minimizer.
// NS: sub-rounds of 64 positions per trip (2: the kernels' iteration of 128 positions; 3, 4: gs_match_wide_kernel, reads of up to
// 192 / 256 positions in ONE trip).  The rank carries its row index in eight bits, so beyond two sub-rounds there are TWO rank rows:
// A for positions 0 .. 143 (read by sub-rounds 0 and 1), B for positions 128 .. 64 NS + 15 with the index counted from 128 (read by
// sub-rounds 2 and 3); the 16 positions both need are written twice.  Layout of the wave's words: [A: GS_ROW][B: GS_ROW, NS > 2 only]
// [canonical 15-mers of all positions: 64 NS + 16].
// LIT: the tail round's "lane < 16" as a literal mask (the FIXED loop of gs_match_kernel: a lane predicate costs a compare whose
// result the compiler keeps across the loop in a spilled scalar pair and reads back per read)
#define GS_WIDE_WORDS(NS) (2 * GS_ROW + 64 * (NS) + 32)
#define GS_ACT(m) __builtin_amdgcn_inverse_ballot_w64(m)  // a wave-level mask as a per-lane condition
template <int KC, int NS = 2, bool LIT = false>
__device__ __forceinline__ void gs_wave_minimizers(const u64 (&Bhi)[NS + 1], const u64 (&Blo)[NS + 1], const uint32_t (&fhi)[NS],
                                                   const uint32_t (&flo)[NS], const uint32_t (&rhi)[NS], const uint32_t (&rlo)[NS], int k,
                                                   int lane, uint32_t *wave_g, int (&p)[NS], uint32_t (&cf)[NS]) {
    static_assert(NS >= 2 && NS <= 4, "two rank rows of 144 positions");
    constexpr bool TWO = NS > 2;
    constexpr int ROWB = GS_ROW, CAN = TWO ? 2 * GS_ROW : GS_ROW;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        // gs_lmer_canon of the k-mer's first 15-mer; its reverse complement is the top 15 bases of the k-mer's (rhi, rlo: the
        // orientation step needs them anyway), and "the smaller of f and r, low bit = f was it" is min(2f + 1, 2r)
        const uint32_t f = ((fhi[s] & 0x7fffu) << GS_MIN_L) | (flo[s] & 0x7fffu);
        const uint32_t rr = ((rhi[s] >> (k - GS_MIN_L)) << GS_MIN_L) | (rlo[s] >> (k - GS_MIN_L));
        const uint32_t c = min((f << 1) | 1u, rr << 1);
        const uint32_t h = gs_canon_hash(c >> 1);
        if (!TWO || s < 2) wave_g[64 * s + lane] = gs_lmer_rank(h, (uint32_t)(64 * s + lane));
        if (TWO && s >= 2) wave_g[ROWB + 64 * (s - 2) + lane] = gs_lmer_rank(h, (uint32_t)(64 * (s - 2) + lane));
        if (TWO && s == 2 && lane < 16) wave_g[128 + lane] = gs_lmer_rank(h, (uint32_t)(128 + lane));
        wave_g[CAN + 64 * s + lane] = c;
    }
    if (LIT ? GS_ACT(0xffffULL) : lane < 16) {
        const uint32_t c = gs_lmer_canon((uint32_t)(Bhi[NS] >> lane) & 0x7fffu, (uint32_t)(Blo[NS] >> lane) & 0x7fffu);
        const uint32_t h = gs_canon_hash(c >> 1);
        if (!TWO)
            wave_g[64 * NS + lane] = gs_lmer_rank(h, (uint32_t)(64 * NS + lane));
        else
            wave_g[ROWB + 64 * (NS - 2) + lane] = gs_lmer_rank(h, (uint32_t)(64 * (NS - 2) + lane));
        wave_g[CAN + 64 * NS + lane] = c;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int w = k - GS_MIN_L + 1;
    // The ranks of a lane's k - 14 positions are read in ONE batch per sub-round (the loads are independent; left to itself the
    // compiler waits after every ds_read2 because of the 64-register budget: nine LDS round trips in a row per sub-round), then
    // folded with min3.
    constexpr int ND = KC ? KC - GS_MIN_L + 1 : 32 - GS_MIN_L;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const uint32_t *row = (TWO && s >= 2) ? wave_g + ROWB + 64 * (s - 2) + lane : wave_g + 64 * s + lane;
        uint32_t g[ND];
#pragma unroll
        for (int d = 0; d < ND; d++) g[d] = (KC || d < w) ? row[d] : 0xffffffffu;
        __builtin_amdgcn_sched_group_barrier(0x100, (ND + 1) / 2, 0);  // the DS reads first ...
        uint32_t mn = g[0];
#pragma unroll
        for (int d = 1; d < ND; d++) mn = g[d] < mn ? g[d] : mn;
        __builtin_amdgcn_sched_group_barrier(0x002, ND, 0);            // ... then the min chain
        const int idx = (int)(mn & 0xffu) + ((TWO && s >= 2) ? 128 : 0);
        cf[s] = wave_g[CAN + idx];
        p[s] = idx - (64 * s + lane);
    }
    __builtin_amdgcn_wave_barrier();  // the rows are rewritten by the next iteration / read
}

// the lanes below n as a wave-level mask: the positions of a sub-round that hold a k-mer, the lanes of a word that hold a base
__device__ __forceinline__ u64 gs_low_mask(int n) { return n >= 64 ? ~0ULL : (n <= 0 ? 0ULL : ((1ULL << n) - 1ULL)); }
// live: the positions of each sub-round that hold a k-mer, gs_low_mask(max - base - 64 s), from a caller that has them already -- they
// depend on the read's length alone, and a batch of one length builds them once per wave (gs_match_kernel<.., FIXED = true>);
// nullptr: derived here from base and max
// CTX: is the gate keyed by gs_gate_ctx_key?  0 never (the launcher has looked), 1 always, 2 ask the store (GsDbDev::mgate_ctx)
// AGG: the unique-k-mer marks of the k-mers that share a record line leave as ONE atomic per line.  A device-scope atomic is
// executed on the memory side of the L2s (eight XCDs, eight L2s): every one is a request to the fabric, and on a store that does not
// fit the caches they were HALF of the kernel's fabric requests (473 M k-mers: 30 read + 36 write requests per read, 61 writes per
// read from the store -- one per first-seen k-mer; tools/huge_lines.py), with the fabric's line rate the bound (0.89).  The lanes of
// a minimizer run OR their offset bits into a word of the wave's LDS rows (free again after the minimizer scan), the lane that owns
// the lowest bit sends the word: ~13 atomics per read from the store instead of ~60.
// LIT: the caller is the FIXED loop -- lane predicates that are constants of the wave are written as literal masks
// NOGATE: the caller's reads have passed the prefilter, or come from a stream the feedback rule found hit-rich (launch_batch,
// DESIGN 4): the minimizer gate, which passes nearly every lane of such a read, is neither addressed, loaded nor tested, and act[s]
// stays "live and not an INVALID window".  The caller has looked: the store has a gate and records (db.mgate, db.rec).  Results do
// not depend on it -- the gate has no false negatives and the record compare is exact.
template <int KC, bool STRIPED, int CTX = 2, bool AGG = false, int NS = 2, bool LIT = false, bool NOGATE = false>
__device__ __forceinline__ void gs_probe_planes(const GsDbDev &db, const u64 (&Bhi)[NS + 1], const u64 (&Blo)[NS + 1],
                                                const u64 (&Bbad)[NS + 1], int base, int max, int lane, int (&node)[NS],
                                                uint32_t *wave_g, const GsMark &mk, const u64 *live = nullptr) {
    static_assert(NS == 2 || !AGG, "the seen-bit accumulators are laid out for two sub-rounds");
    static_assert(!NOGATE || (LIT && !STRIPED && CTX == 0 && NS == 2), "every other variant uses the hint bits of the gate word");
    const int k = KC ? KC : db.k;  // KC = compile-time k of the specialised kernels (0: any k)
    const uint32_t kmask = (1u << k) - 1u;
    const uint32_t vmask2 = 2u * ((1u << db.vbits) - 1u);
    const int shift_rem = (int)db.vbits + 3;
    const uint32_t bmask = (uint32_t)db.bucket_mask;  // n_buckets <= 2^29
    bool any_bad = false;
#pragma unroll
    for (int w = 0; w <= NS; w++) any_bad = any_bad || Bbad[w] != 0;
    uint32_t fhi[NS], flo[NS];
    // Which lanes hold a live k-mer is kept as a wave-level MASK (a scalar register pair), not as a per-lane flag: "position < max"
    // is a mask the scalar unit builds from the read length, every later condition is one vector compare whose result is a
    // mask already, and a mask conditions a lane directly (inverse ballot) -- no flag is materialised in a vector register and
    // compared again.
    u64 act[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const u64 vm = live != nullptr ? live[s] : gs_low_mask(max - base - 64 * s);  // valid positions of this sub-round
        fhi[s] = (uint32_t)gs_funnel(Bhi[s], Bhi[s + 1], lane) & kmask;
        flo[s] = (uint32_t)gs_funnel(Blo[s], Blo[s + 1], lane) & kmask;
        act[s] = vm;
        node[s] = GS_ACT(vm) ? GS_NODE_MISS : GS_NODE_NONE;
        if (any_bad) {  // almost every read is clean: the per-lane window test sits behind a wave-uniform branch
            const u64 wb = __ballot(((uint32_t)gs_funnel(Bbad[s], Bbad[s + 1], lane) & kmask) != 0u) & vm;
            act[s] = vm & ~wb;
            node[s] = GS_ACT(wb) ? GS_NODE_INVALID : node[s];
        }
    }
    if (NOGATE || db.mgate != nullptr) {
        // minimizer gate: lanes that share a minimizer read the same gate word -> one request
        int mp[NS];
        uint32_t cf[NS];
        GS_STAMP(2, fhi[1] ^ flo[1])
        uint32_t rhi[NS], rlo[NS];  // reverse complement of the k-mer
#pragma unroll
        for (int s = 0; s < NS; s++) {
            rhi[s] = __brev(fhi[s]) >> (32 - k);
            rlo[s] = (__brev(flo[s]) >> (32 - k)) ^ kmask;
        }
        gs_wave_minimizers<KC, NS, LIT>(Bhi, Blo, fhi, flo, rhi, rlo, k, lane, wave_g, mp, cf);
        GS_STAMP(3, cf[0] ^ cf[1])
        uint32_t gh[NS], ohi[NS], olo[NS];
        int j[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) gs_min_oriented_cf(cf[s], fhi[s], flo[s], rhi[s], rlo[s], k, mp[s], gh[s], ohi[s], olo[s], j[s]);
        // Lanes that look into their minimizer's second bucket as well.  Every store carries the hint bits (gs_mgate_hint); they
        // are USED where a record line is dear -- a context-keyed store (hundreds of millions of k-mers, lines from HBM) and a
        // striped one (lines over xGMI) --: on a store whose records sit in the caches the second line costs less than the
        // test (measured on configs[1]: 6.74 ms without, 6.94 ms with it; 47 M store 8.66 / 8.68; 473 M store 15.39 / 15.03).
        const bool use_hint = STRIPED || CTX == 1 || (CTX == 2 && db.mgate_ctx);
        u64 two[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) two[s] = ~0ULL;
        if (!NOGATE && (GS_ABLATE & 4) == 0) {
            // the gate words of both sub-rounds are requested together (lanes without a live k-mer read word 0): one round
            // trip, no exec-mask regions
            uint32_t gw[NS];
            uint32_t gk[NS];  // what the gate is keyed by: the minimizer, or (big stores) the minimizer + four bases next to it
#pragma unroll
            for (int s = 0; s < NS; s++) gk[s] = (CTX == 1 || (CTX == 2 && db.mgate_ctx)) ? gs_gate_ctx_key(gh[s], ohi[s], olo[s], j[s], k) : gh[s];
#pragma unroll
            for (int s = 0; s < NS; s++)
                gw[s] = db.mgate[GS_ACT(act[s]) ? ((CTX == 1 || (CTX == 2 && db.mgate_ctx)) ? gs_mgate_word_ctx(gk[s], db.mgate_bits) : gs_mgate_word(gk[s], db.mgate_bits)) : 0u];
#pragma unroll
            for (int s = 0; s < NS; s++) {
                const uint32_t bits = gs_mgate_bits(gk[s]);
                act[s] &= __ballot((gw[s] & bits) == bits);  // no false negatives
                if (use_hint) two[s] = __ballot((gw[s] & gs_mgate_hint(gk[s])) != 0u);  // a window of this key may sit in the second bucket
            }
            GS_STAMP(4, gw[0] ^ gw[1])
        }
        if (GS_ABLATE & 6) {  // keep the values alive, look nothing up
#pragma unroll
            for (int s = 0; s < NS; s++)
                if (GS_ACT(act[s]) && (gh[s] ^ ohi[s] ^ olo[s] ^ (uint32_t)j[s]) == 0x12345u) node[s] = 0;
            return;
        }
        if (NOGATE || STRIPED || db.rec != nullptr) {
            // ---- super-k-mer records: per candidate bucket of the minimizer one 16-byte load of the window planes + the
            // 8-byte word that holds this offset's value.  The first bucket always; the second one only where the gate word
            // carries the key's hint bit (two windows in three sit in their first bucket: a third fewer line requests, which
            // is what bounds a store that does not fit the caches).  Both loads of a sub-round are in flight together and the
            // compares are straight-line code (bitwise, no short-circuit branches: every branch is an exec-mask save /
            // restore on the scalar unit, which this kernel keeps as busy as the vector unit)
            u64 any_act = 0;
#pragma unroll
            for (int s = 0; s < NS; s++) any_act |= act[s];
            if (any_act == 0) return;  // nothing passed the gate: a read that is not from the store
            if (AGG && mk.count_unique) {  // accumulators of the seen bits: 80 minimizer positions x 2 buckets per sub-round
#pragma unroll
                for (int q = 0; q < 5; q++) wave_g[64 * q + lane] = 0u;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            // (Tried in round 3 and dropped, twice: touching sub-round 1's lines -- one dword each -- before sub-round 0's loads go
            // out, so that the second record round trip (3 400 + 3 200 of 24 900 wave cycles per read on the 473 M-k-mer store,
            // tools/phase_times.sh huge) is an L2 hit.  With plain loads, which the compiler is free to sink: configs[1] 6.80 ->
            // 7.05 ms, 47 M store 8.72 -> 9.08, 473 M store 15.0 -> 15.2.  With loads the compiler does not see (inline asm, issued
            // first for certain; big stores only): 473 M store 15.0 -> 15.2 ms, striped 7.24 -> 7.40.  The round trip that was
            // taken out does not come off the kernel's time.)
#pragma unroll
            for (int s = 0; s < NS; s++) {
                bool pending = false;
                if (GS_ACT(act[s])) {
                    const uint32_t jj = (uint32_t)j[s];
                    const int jw = (int)(jj * 11u) >> 5;  // j / 3 for j <= 16
                    const uint32_t b0 = gs_rec_bucket(gh[s], db.rec_bits, 0), b1 = gs_rec_bucket(gh[s], db.rec_bits, 1);
                    // the stripe's (biased) base pointer from the wave's copy of the table, behind the hash rows
                    const u64 *r0 = (STRIPED ? gs_rec_stripe(db, wave_g, b0) : db.rec) + (u64)b0 * GS_REC_WORDS;
                    gs_u64x2 A1 = {0, 0};  // (no valid bit: matches nothing)
                    u64 V1 = 0;
                    if (!use_hint || GS_ACT(two[s])) {
                        const u64 *r1 = (STRIPED ? gs_rec_stripe(db, wave_g, b1) : db.rec) + (u64)b1 * GS_REC_WORDS;
                        A1 = *reinterpret_cast<const gs_u64x2 *>(r1);
                        V1 = r1[2 + jw];
                    }
                    const gs_u64x2 A0 = *reinterpret_cast<const gs_u64x2 *>(r0);
                    const u64 V0 = r0[2 + jw];
                    // window bits [j, j + k) of a plane: j + k <= 2k - 15, so the seen / valid bits above the window stay out
                    // of the low k bits of the shifted word; one 32-bit funnel shift (j <= 16) per plane
                    const uint32_t x0 = __builtin_amdgcn_alignbit((uint32_t)(A0.x >> 32), (uint32_t)A0.x, jj);
                    const uint32_t y0 = __builtin_amdgcn_alignbit((uint32_t)(A0.y >> 32), (uint32_t)A0.y, jj);
                    const uint32_t x1 = __builtin_amdgcn_alignbit((uint32_t)(A1.x >> 32), (uint32_t)A1.x, jj);
                    const uint32_t y1 = __builtin_amdgcn_alignbit((uint32_t)(A1.y >> 32), (uint32_t)A1.y, jj);
                    const uint32_t fbit = 1u << (GS_REC_WIN_BITS - 32 + jj);  // seen (w0) / valid (w1) bit of offset j, high dword
                    const bool ok0 = ((((x0 ^ ohi[s]) | (y0 ^ olo[s])) & kmask) == 0) & (((uint32_t)(A0.y >> 32) & fbit) != 0);
                    const bool ok1 = ((((x1 ^ ohi[s]) | (y1 ^ olo[s])) & kmask) == 0) & (((uint32_t)(A1.y >> 32) & fbit) != 0);
                    const bool hit = ok0 | ok1;  // (an eligible k-mer is filed in exactly one window)
                    const u64 V = ok0 ? V0 : V1;
                    const uint32_t seen_hi = ok0 ? (uint32_t)(A0.x >> 32) : (uint32_t)(A1.x >> 32);
                    const uint32_t rb = ok0 ? b0 : b1;
                    const int val = (int)((V >> (GS_REC_VAL_BITS * ((int)jj - 3 * jw))) & (GS_REC_MAX_VALUES - 1));
                    node[s] = hit ? val : node[s];
                    if (hit) {
                        if (STRIPED && AGG) {
                            if (mk.count_unique && ((mk.rec_seen[rb] >> jj) & 1u) == 0) {
                                uint32_t *acc = wave_g + GS_ROW * s + 2 * (mp[s] + lane) + (ok0 ? 0 : 1);
                                atomicOr(acc, 1u << jj);
                                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                                const uint32_t w = *(volatile uint32_t *)acc;
                                if ((w & (0u - w)) == (1u << jj)) atomicOr(mk.rec_seen + rb, w);
                            }
                        } else if (STRIPED) {
                            if (mk.count_unique && ((mk.rec_seen[rb] >> jj) & 1u) == 0) atomicOr(mk.rec_seen + rb, 1u << jj);
                        } else if (AGG) {
                            if (mk.count_unique && (seen_hi & fbit) == 0) {
                                // (the lanes of a minimizer occurrence share both buckets; occurrence = mp + lane inside the sub-round, < 80)
                                uint32_t *acc = wave_g + GS_ROW * s + 2 * (mp[s] + lane) + (ok0 ? 0 : 1);
                                atomicOr(acc, 1u << jj);
                                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                                const uint32_t w = *(volatile uint32_t *)acc;
                                if ((w & (0u - w)) == (1u << jj))  // the owner of the lowest bit sends the run's bits
                                    atomicOr(const_cast<u64 *>(db.rec) + (u64)rb * GS_REC_WORDS, (u64)w << GS_REC_WIN_BITS);
                            }
                        } else if (mk.count_unique && (seen_hi & fbit) == 0)
                            atomicOr(const_cast<u64 *>(db.rec) + (u64)rb * GS_REC_WORDS, 1ULL << (GS_REC_WIN_BITS + jj));
                        if (mk.hit_counts != nullptr)
                            atomicAdd(mk.hit_counts + ((u64)(bmask + 1u) * GS_SLOTS_PER_BUCKET + (u64)rb * GS_REC_SLOTS + (u64)jj), 1u);
                    }
                    pending = !hit & (((V0 | V1) & GS_REC_MORE) != 0);
                }
                GS_STAMP(8 + 2 * s, node[s])  // (phase 8 / 10: the record lines of sub-round 0 / 1)
                // a k-mer whose window found no bucket (or that has two strand views) lives in the table
                if (__ballot(pending) != 0) {
                    const u64 h = gs_kmer_hash(ohi[s], olo[s], k, kmask);
                    gs_lookup_rest<true, STRIPED>(db, (uint32_t)h & bmask, (h >> db.bucket_bits) << shift_rem, vmask2, pending, node[s], mk, wave_g);
                }
                GS_STAMP(9 + 2 * s, node[s])  // (phase 9 / 11: its walk of the overflow table)
            }
            return;
        }
    }
    // ---- the ordinary table: one 64-byte bucket line per k-mer (stores without records: k < 19, partitions, > 2^21 values)
    uint32_t bkt[NS];
    u64 want[NS];
    GsHalf bk[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const u64 h = gs_kmer_hash(fhi[s], flo[s], k, kmask);
        bkt[s] = (uint32_t)h & bmask;
        want[s] = (h >> db.bucket_bits) << shift_rem;
        if (db.mgate == nullptr && db.gate != nullptr) {  // word gate (L2-resident), no false negatives
            bool pass = false;
            if (GS_ACT(act[s])) {
                const u64 gbits = gs_gate_field_bits((uint32_t)(h >> GS_GATE_FIELD_SHIFT));
                pass = (db.gate[(h >> db.bucket_bits) & db.gate_mask] & gbits) == gbits;
            }
            act[s] = __ballot(pass);
        }
        if (GS_ACT(act[s])) gs_load_half(db.table, bkt[s], 0, bk[s]);  // both sub-rounds' loads in flight together
    }
#pragma unroll
    for (int s = 0; s < NS; s++) {
        bool pending = false;
        if (GS_ACT(act[s])) {
            int vs = -1, sl = 0;
            const bool done = gs_match_half(bk[s], want[s], vmask2, vs, sl);
            if (vs >= 0) gs_take_hit<false>(db, bkt[s] * GS_SLOTS_PER_BUCKET + sl, vs, node[s], mk);
            pending = !done;
        }
        gs_lookup_rest<false, false>(db, bkt[s], want[s], vmask2, pending, node[s], mk, wave_g);
    }
}

// STRIPED: the record table is split over several devices (GsDbDev::rec_biased); every wave keeps the stripe pointers in
// LDS behind its hash rows, where a lane picks the one of its bucket with a single ds_read
#define GS_STRIPE_TABLE(kernarg)                                                                                        \
    if (STRIPED) {                                                                                                       \
        if (lane < 2 * GS_MAX_STRIPES)                                                                                   \
            reinterpret_cast<const u64 **>(s_g[wave_in_block] + 2 * GS_ROW)[lane] =                                      \
                lane < GS_MAX_STRIPES ? (kernarg)->db.rec_biased[lane] : (kernarg)->db.tab_biased[lane - GS_MAX_STRIPES]; \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                           \
        __builtin_amdgcn_wave_barrier();                                                                                 \
    }
