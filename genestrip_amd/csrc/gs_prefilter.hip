// gs_prefilter.hip -- the 15-mer filter of a store and the kernel that keeps reads without a stored k-mer off the match kernel's
// waves (gs_prefilter.h has the argument and the test itself; DESIGN 4, "Sampled 15-mer prefilter").
//   gs_pf_build_kernel   one sweep over the finished store (record lines, then table slots): every stored k-mer sets the canonical
//                        codes of its k - 14 15-mers in both levels.  OR is commutative: the bits do not depend on scheduling.
//   gs_pf_count_kernel   |S| = the set bits of the exact level
//   gs_pf_kernel         a batch of one read length, ONE READ PER LANE: the wave copies its 64 reads (64 L contiguous bytes) into
//                        LDS with 16-byte loads, every lane then walks the samples of its own read.  A workgroup takes
//                        GS_PF_ROUNDS x 256 reads and reserves the places of its survivors with ONE atomic (atomics on one
//                        address run one after the other, ~11 ns each: one per wave and round would cost more than the kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gs_launch.h"
#include "gs_layout.h"
#include "gs_params.h"
#include "gs_prefilter.h"

typedef unsigned long long u64;

#define GS_PF_BLOCK 256
#define GS_PF_ROUNDS 8
#define GS_PF_READS (GS_PF_BLOCK * GS_PF_ROUNDS)

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

// bytes of LDS one wave needs for 64 reads of L bytes: the reads, up to 15 bytes in front of them (the copy starts at a 16-byte
// boundary of global memory), and the four bytes behind the last sample's last dword
__host__ __device__ static inline uint32_t gs_pf_wave_bytes(int L) { return (uint32_t)((64 * L + 15 + 4 + 15) & ~15) + 16u; }

__global__ __launch_bounds__(GS_PF_BLOCK) void gs_pf_kernel(GsPrefilterParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pf_lds[];
    __shared__ unsigned int s_wave[GS_PF_BLOCK / 64];
    __shared__ unsigned int s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = P.L, k = P.k;
    const int w = gs_pf_stride(k), m = gs_pf_samples(L, k);
    unsigned char *buf = pf_lds + (size_t)wave * gs_pf_wave_bytes(L);
    const uint32_t *buf32 = reinterpret_cast<const uint32_t *>(buf);
    const uintptr_t seq_lo = (uintptr_t)P.seq, seq_hi = seq_lo + (uintptr_t)P.n_reads * (uintptr_t)L;
    const int64_t b0 = (int64_t)blockIdx.x * GS_PF_READS;
    uint32_t passed = 0;  // bit j: the lane's read of round j goes on to the match kernel
    for (int j = 0; j < GS_PF_ROUNDS; j++) {
        const int64_t r0 = b0 + (int64_t)j * GS_PF_BLOCK + 64 * wave;  // the wave's first read of this round
        if (r0 >= P.n_reads) break;                                   // (wave-uniform)
        const int nr = P.n_reads - r0 < 64 ? (int)(P.n_reads - r0) : 64;
        const uintptr_t g0 = seq_lo + (uintptr_t)r0 * (uintptr_t)L;
        const uintptr_t a0 = g0 & ~(uintptr_t)15;
        const int delta = (int)(g0 - a0);
        const int chunks = (delta + nr * L + 15) >> 4;  // <= (15 + 64 L + 15) / 16: inside the wave's buffer
        for (int c = lane; c < chunks; c += 64) {
            const uintptr_t a = a0 + 16u * (uintptr_t)c;
            uint4 v;
            if (a >= seq_lo && a + 16 <= seq_hi)
                v = *reinterpret_cast<const uint4 *>(a);
            else {  // the 16 bytes straddle an end of the batch: only its own bytes are read
                uint32_t x[4] = {0, 0, 0, 0};
                for (int i = 0; i < 16; i++)
                    if (a + i >= seq_lo && a + i < seq_hi) x[i >> 2] |= (uint32_t) * reinterpret_cast<const uint8_t *>(a + i) << (8 * (i & 3));
                v = make_uint4(x[0], x[1], x[2], x[3]);
            }
            *reinterpret_cast<uint4 *>(buf + 16 * c) = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        bool pass = false;
        if (lane < nr) {
            const int at = delta + lane * L;
            for (int i = 0; i < m && !pass; i++) {
                const int b = at + i * w;  // i w <= L - 15: the 15 bytes lie inside the lane's read
                const uint32_t *q = buf32 + (b >> 2);
                const uint32_t sh = (uint32_t)b & 3u;
                const uint32_t x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3], x4 = q[4];
                const uint32_t d0 = __builtin_amdgcn_alignbyte(x1, x0, sh), d1 = __builtin_amdgcn_alignbyte(x2, x1, sh);
                const uint32_t d2 = __builtin_amdgcn_alignbyte(x3, x2, sh), d3 = __builtin_amdgcn_alignbyte(x4, x3, sh);
                pass = gs_pf_sample_in(P.l1, P.l2, d0, d1, d2, d3);
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
    for (int bit = 0; bit < 4; bit++) {  // (mine <= GS_PF_ROUNDS = 8)
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
    const int64_t grid = (P->n_reads + GS_PF_READS - 1) / GS_PF_READS;
    hipLaunchKernelGGL(gs_pf_kernel, dim3((unsigned)grid), dim3(GS_PF_BLOCK), (GS_PF_BLOCK / 64) * gs_pf_wave_bytes(P->L), stream, *P);
    return hipGetLastError();
}
