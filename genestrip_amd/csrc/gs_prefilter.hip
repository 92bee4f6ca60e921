// gs_prefilter.hip -- the 15-mer filter of a store and the kernel that keeps reads without a stored k-mer off the match kernel's
// waves (gs_prefilter.h has the argument and the test itself; DESIGN 4, "Sampled 15-mer prefilter").
//   gs_pf_build_kernel   one sweep over the finished store (record lines, then table slots): every stored k-mer sets the canonical
//                        codes of its k - 14 15-mers in both levels.  OR is commutative: the bits do not depend on scheduling.
//   gs_pf_count_kernel   |S| = the set bits of the exact level
//   gs_pf_kernel         a batch of one read length, ONE READ PER LANE: the wave copies its 64 reads (64 L contiguous bytes) into
//                        LDS with 16-byte loads, all of a lane's loads issued before the first is used; every lane then tests
//                        the samples of its own read: sample 0 alone (it decides nearly every read from the store's genomes),
//                        the others eight at a time -- eight codes, eight level-one loads in flight together, then the exact
//                        level for the level-one passes only, the lanes of the wave stepping together (gs_prefilter.h).  A
//                        workgroup takes GS_PF_ROUNDS x 256 reads and reserves the places of its survivors with ONE atomic
//                        (atomics on one address run one after the other, ~11 ns each: one per wave and round would cost
//                        more than the kernel).  What was measured and dropped: DESIGN 4.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gs_launch.h"
#include "gs_layout.h"
#include "gs_params.h"
#include "gs_prefilter.h"

typedef unsigned long long u64;

#define GS_PF_BLOCK 256
#define GS_PF_ROUNDS 4
#define GS_PF_READS (GS_PF_BLOCK * GS_PF_ROUNDS)
#define GS_PF_MIN_L 32   // a round of one read still has a whole second 16-byte piece (gs_pf_stage_load)
#define GS_PF_MAX_L 158  // = GS_MAX_K + 127, the longest read of the FIXED loop
#define GS_PF_PIECES 10  // 16-byte pieces per lane and round: 64 x 10 x 16 bytes hold 15 + 64 GS_PF_MAX_L + 15
static_assert(15 + 64 * GS_PF_MAX_L + 15 <= 64 * GS_PF_PIECES * 16, "a wave round is at most GS_PF_PIECES pieces per lane");

__device__ __forceinline__ void gs_pf_set(uint32_t *words, uint32_t bit) {
    uint32_t *w = words + (bit >> 5);
    const uint32_t m = 1u << (bit & 31);
    if ((*w & m) == 0) atomicOr(w, m);  // a set bit costs no atomic (a stale 0 only costs one more)
}

__device__ __forceinline__ void gs_pf_put(const GsPrefilterBuildParams &P, uint32_t fh, uint32_t fl) {
    const uint32_t c = gs_lmer_canon(fh & 0x7fffu, fl & 0x7fffu) >> 1;
    gs_pf_set(P.l2, c);
    gs_pf_set(P.l1, gs_pf_l1_bit(c));
}

__global__ __launch_bounds__(GS_PF_BLOCK) void gs_pf_build_kernel(GsPrefilterBuildParams P) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int w = gs_pf_stride(P.k);
    // record lines: the window's 15-mer positions that a valid k-mer covers -- offset j covers j .. j + w - 1 -- each once
    for (int64_t line = t0; line < P.n_rec; line += stride) {
        const u64 w0 = P.rec[(size_t)line * GS_REC_WORDS], w1 = P.rec[(size_t)line * GS_REC_WORDS + 1];
        const u64 whi = w0 & ((1ULL << GS_REC_WIN_BITS) - 1), wlo = w1 & ((1ULL << GS_REC_WIN_BITS) - 1);
        uint32_t valid = (uint32_t)(w1 >> GS_REC_WIN_BITS) & ((1u << w) - 1u);
        u64 cover = 0;
        for (; valid; valid &= valid - 1) cover |= ((1ULL << w) - 1ULL) << __builtin_ctz(valid);
        for (; cover; cover &= cover - 1) {
            const int p = __builtin_ctzll(cover);
            gs_pf_put(P, (uint32_t)(whi >> p), (uint32_t)(wlo >> p));
        }
    }
    // table slots (slot = rem | disp | value + 1 | seen; 0 = empty)
    const uint32_t vmask = (1u << P.vbits) - 1u;
    const u64 bmask = (1ULL << P.bucket_bits) - 1;
    const uint32_t kmask = (uint32_t)((1ULL << P.k) - 1);
    for (int64_t t = t0; t < P.n_tab * GS_SLOTS_PER_BUCKET; t += stride) {
        const u64 s = P.tab[t];
        if (((uint32_t)(s >> 1) & vmask) == 0) continue;
        const u64 bucket = (u64)(t / GS_SLOTS_PER_BUCKET);
        const u64 disp = (s >> (P.vbits + 1)) & 3u, rem = s >> (P.vbits + 3);
        uint32_t a, b;
        gs_unmix_planes((rem << P.bucket_bits) | ((bucket - disp) & bmask), a, b);
        a &= kmask;
        b &= kmask;
        for (int d = 0; d < w; d++) gs_pf_put(P, a >> d, b >> d);
    }
}

__global__ __launch_bounds__(GS_PF_BLOCK) void gs_pf_count_kernel(const uint32_t *l2, unsigned long long *count) {
    __shared__ unsigned int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    unsigned int n = 0;
    const uint4 *p = reinterpret_cast<const uint4 *>(l2);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < GS_PF_L2_WORDS / 4; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 v = p[i];
        n += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
    if (n) atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(count, (unsigned long long)s_n);
}

// one wave round: reads r0 .. r0 + nr - 1 of the batch, and where their bytes lie (gs_pf_copy_pieces, gs_pf_piece_range)
struct GsPfRound {
    int64_t r0;
    const uint8_t *a0;  // the 16-byte boundary of global memory at or in front of the first read
    int nr, delta, pieces;
    bool first, last;  // the round holds the first / the last read of the batch
};
__device__ __forceinline__ GsPfRound gs_pf_round(const GsPrefilterParams &P, int64_t r0) {
    GsPfRound R;
    R.r0 = r0;
    R.nr = P.n_reads - r0 < 64 ? (int)(P.n_reads - r0) : 64;
    const uintptr_t g0 = (uintptr_t)P.seq + (uintptr_t)r0 * (uintptr_t)P.L;
    R.delta = (int)(g0 & 15);
    R.a0 = P.seq + (r0 * (int64_t)P.L - R.delta);  // (offsets from the kernel's own argument: global loads, not flat ones)
    R.pieces = gs_pf_copy_pieces(R.delta, R.nr, P.L);  // <= (15 + 64 L + 15) / 16 <= 64 GS_PF_PIECES: inside the wave's buffer
    R.first = r0 == 0;
    R.last = r0 + R.nr == P.n_reads;
    return R;
}

// the lane's pieces lane, lane + 64, .. of a round, global memory -> registers.  Every lane issues all GS_PF_PIECES 16-byte loads
// with no branch between them (a lane without a whole piece at that place loads piece 1, which is whole in every round: a round
// holds at least GS_PF_MIN_L = 32 bytes behind at most 15); only a piece cut at an end of the batch takes the byte-wise path, and reads its own bytes only.
__device__ __forceinline__ void gs_pf_stage_load(const GsPfRound &R, int L, int lane, uint4 (&v)[GS_PF_PIECES]) {
    uint32_t cut = 0;
#pragma unroll
    for (int i = 0; i < GS_PF_PIECES; i++) {
        const int c = lane + 64 * i;
        int lo, hi;
        gs_pf_piece_range(c, R.delta, R.nr, L, R.first, R.last, &lo, &hi);
        const bool mine = c < R.pieces, whole = hi - lo == 16;
        v[i] = *reinterpret_cast<const uint4 *>(R.a0 + 16 * (mine && whole ? c : 1));
        if (mine && !whole) cut |= 1u << i;
    }
    for (; cut; cut &= cut - 1) {  // (at most two lanes of the batch's first and last wave round)
        const int ci = __builtin_ctz(cut), c = lane + 64 * ci;
        int lo, hi;
        gs_pf_piece_range(c, R.delta, R.nr, L, R.first, R.last, &lo, &hi);
        uint32_t x[4] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const int b = 16 * c + t;
            if (b >= lo && b < hi) x[t >> 2] |= (uint32_t)R.a0[b] << (8 * (t & 3));
        }
#pragma unroll
        for (int i = 0; i < GS_PF_PIECES; i++)
            if (i == ci) v[i] = make_uint4(x[0], x[1], x[2], x[3]);
    }
}
__device__ __forceinline__ void gs_pf_stage_write(const GsPfRound &R, int lane, const uint4 (&v)[GS_PF_PIECES], unsigned char *buf) {
#pragma unroll
    for (int i = 0; i < GS_PF_PIECES; i++) {
        const int c = lane + 64 * i;
        if (c < R.pieces) *reinterpret_cast<uint4 *>(buf + 16 * c) = v[i];
    }
}

// the 15 bytes at buffer byte b, first one in byte 0 of d0
__device__ __forceinline__ void gs_pf_sample_bytes(const uint32_t *buf32, int b, uint32_t &d0, uint32_t &d1, uint32_t &d2, uint32_t &d3) {
    const uint32_t *q = buf32 + (b >> 2);
    const uint32_t sh = (uint32_t)b & 3u;
    const uint32_t x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3], x4 = q[4];
    d0 = __builtin_amdgcn_alignbyte(x1, x0, sh);
    d1 = __builtin_amdgcn_alignbyte(x2, x1, sh);
    d2 = __builtin_amdgcn_alignbyte(x3, x2, sh);
    d3 = __builtin_amdgcn_alignbyte(x4, x3, sh);
}

// (LDS allows 16 waves per CU = 4 per SIMD: the registers may go up to 128)
__global__ __launch_bounds__(GS_PF_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void gs_pf_kernel(GsPrefilterParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pf_lds[];
    __shared__ unsigned int s_wave[GS_PF_BLOCK / 64];
    __shared__ unsigned int s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = P.L, k = P.k;
    const int w = gs_pf_stride(k), m = gs_pf_samples(L, k);
    unsigned char *buf = pf_lds + (size_t)wave * gs_pf_wave_bytes(L);
    const uint32_t *buf32 = reinterpret_cast<const uint32_t *>(buf);
    const int64_t b0 = (int64_t)blockIdx.x * GS_PF_READS;
    uint32_t passed = 0;  // bit j: the lane's read of round j goes on to the match kernel
    uint4 stage[GS_PF_PIECES];  // the lane's pieces of the round
    const int64_t r00 = b0 + 64 * wave;  // the wave's first read of round 0
    for (int j = 0; j < GS_PF_ROUNDS; j++) {
        const int64_t r0 = r00 + (int64_t)j * GS_PF_BLOCK;  // the wave's first read of this round
        if (r0 >= P.n_reads) break;                          // (wave-uniform)
        const GsPfRound R = gs_pf_round(P, r0);
        gs_pf_stage_load(R, L, lane, stage);
        gs_pf_stage_write(R, lane, stage, buf);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        bool pass = false;
        if (lane < R.nr) {
            const int at = R.delta + lane * L;
            // sample 0 on its own: it decides nearly every read that comes from the store's genomes, at one level-one load
            {
                uint32_t d0, d1, d2, d3;
                gs_pf_sample_bytes(buf32, at, d0, d1, d2, d3);
                const uint32_t c = gs_pf_canon15_dot(d0, d1, d2, d3), l1w = P.l1[gs_pf_l1_bit(c) >> 5];
                pass = gs_pf_group_decide(gs_pf_group_l1(&c, &l1w, 1), [&](int) {
                           return ((P.l2[c >> 5] >> (c & 31)) & 1u) != 0 && gs_pf_bad15(d0, d1, d2, d3) == 0;
                       }) >= 0;
            }
            // the others in groups (a per-lane loop: the wave leaves it when every lane is decided or out of samples)
            for (int s0 = 1; s0 < m && !pass; s0 += GS_PF_GROUP) {
                const int ng = gs_pf_group_size(s0, m);
                uint32_t codes[GS_PF_GROUP], l1w[GS_PF_GROUP];
#pragma unroll
                for (int i = 0; i < GS_PF_GROUP; i++) {  // (past the group's end: its last sample again, masked out below)
                    const int b = at + (s0 + (i < ng ? i : ng - 1)) * w;  // s w <= L - 15: the 15 bytes lie inside the lane's read
                    uint32_t d0, d1, d2, d3;
                    gs_pf_sample_bytes(buf32, b, d0, d1, d2, d3);
                    codes[i] = gs_pf_canon15_dot(d0, d1, d2, d3);
                }
#pragma unroll
                for (int i = 0; i < GS_PF_GROUP; i++) l1w[i] = P.l1[i < ng ? gs_pf_l1_bit(codes[i]) >> 5 : 0u];  // (word 0: one line for the wave)
                const uint32_t todo = gs_pf_group_l1(codes, l1w, GS_PF_GROUP) & ((1u << ng) - 1u);
                pass = gs_pf_group_decide(todo, [&](int i) {  // (the code again from the bytes: a lane-dependent index would send codes[] to scratch)
                           uint32_t d0, d1, d2, d3;
                           gs_pf_sample_bytes(buf32, at + (s0 + i) * w, d0, d1, d2, d3);
                           const uint32_t c = gs_pf_canon15_dot(d0, d1, d2, d3);
                           return ((P.l2[c >> 5] >> (c & 31)) & 1u) != 0 && gs_pf_bad15(d0, d1, d2, d3) == 0;
                       }) >= 0;
            }
            if (pass)
                passed |= 1u << j;
            else {
                if (P.class_vi) P.class_vi[r0 + lane] = -1;
                if (P.flags) P.flags[r0 + lane] = 0;
            }
        }
        __builtin_amdgcn_wave_barrier();  // the buffer is rewritten by the next round
    }
    // places: the lane's survivors behind those of the lower lanes, the wave's behind the lower waves', the workgroup's by one atomic
    const int mine = __popc(passed);
    int before = 0, total = 0;
    const u64 lt = (1ULL << lane) - 1ULL;
    for (int bit = 0; bit < 4; bit++) {  // (mine <= GS_PF_ROUNDS = 4)
        const u64 bm = __ballot((mine >> bit) & 1);
        before += __popcll(bm & lt) << bit;
        total += __popcll(bm) << bit;
    }
    if (lane == 0) s_wave[wave] = (unsigned int)total;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int sum = 0;
        for (int i = 0; i < GS_PF_BLOCK / 64; i++) sum += s_wave[i];
        s_base = sum ? atomicAdd(P.count, sum) : 0u;
    }
    __syncthreads();
    unsigned int place = s_base + (unsigned int)before;
    for (int i = 0; i < wave; i++) place += s_wave[i];
    for (uint32_t pm = passed; pm; pm &= pm - 1)
        P.list[place++] = (uint32_t)(b0 + (int64_t)__builtin_ctz(pm) * GS_PF_BLOCK + threadIdx.x);
}
static_assert(GS_PF_ROUNDS <= 15, "the place scan takes four bits per lane");

extern "C" hipError_t gs_launch_prefilter_build(const GsPrefilterBuildParams *P, int n_cu, hipStream_t stream) {
    const int64_t threads = std::max<int64_t>(P->n_rec, P->n_tab * GS_SLOTS_PER_BUCKET);
    if (threads > 0) {
        int64_t grid = (threads + GS_PF_BLOCK - 1) / GS_PF_BLOCK;
        if (grid > (int64_t)n_cu * 32) grid = (int64_t)n_cu * 32;
        hipLaunchKernelGGL(gs_pf_build_kernel, dim3((unsigned)grid), dim3(GS_PF_BLOCK), 0, stream, *P);
    }
    hipLaunchKernelGGL(gs_pf_count_kernel, dim3((unsigned)(n_cu * 8)), dim3(GS_PF_BLOCK), 0, stream, P->l2, P->count);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_prefilter(const GsPrefilterParams *P, hipStream_t stream) {
    if (P->n_reads <= 0) return hipSuccess;
    if (P->L < GS_PF_MIN_L || P->L > GS_PF_MAX_L || P->L < P->k) return hipErrorInvalidValue;
    const int64_t grid = (P->n_reads + GS_PF_READS - 1) / GS_PF_READS;
    hipLaunchKernelGGL(gs_pf_kernel, dim3((unsigned)grid), dim3(GS_PF_BLOCK), (GS_PF_BLOCK / 64) * gs_pf_wave_bytes(P->L), stream, *P);
    return hipGetLastError();
}
