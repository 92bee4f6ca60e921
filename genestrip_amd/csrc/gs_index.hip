// gs_index.hip -- the index goal on the device (include/gsgpu.h, gs_bloom_build_db): BloomIndexGoal.doMakeThis
// (C/goals/refseq/BloomIndexGoal.java:66-113) over a handle's store.  One walk (gs_decode.h, the walk of gs_ex_decode_kernel)
// selects the stored k-mers whose value is requested (one bit per value) and puts each into the filter:
//   XOR / Murmur  AbstractKMerBloomFilter.putLong :196-203: bit abs(h_i(kmer) % bits) for every hash i
//   Blocked       BlockedKMerBloomFilter.putLong :109-125: two words of one bucket run
// No key or value array is written and nothing is sorted.  The same kernel with put == 0 only counts (the filter is sized by
// the count); the put pass counts again and the host compares.  OR is commutative: the words do not depend on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_absmod.h"
#include "gs_decode.h"
#include "gs_launch.h"
#include "gs_layout.h"
#include "gs_params.h"

#define GS_IX_BLOCK 256
#define GS_IX_QUEUE 288       // selected keys of one wave step: 16 lines x (3 lanes x GS_EX_MAX_PER_LANE)
#define GS_IX_MAX_HASHES 64
#define GS_IX_LDS_WORDS 8192  // the requested bitmap travels in LDS up to 2^18 values (32 KiB), else it is read from global memory

// LDS: per wave a queue of GS_IX_QUEUE keys, the hash factors, then (BM_LDS) the requested bitmap
#define GS_IX_LDS_FIXED (((GS_IX_BLOCK / 64) * GS_IX_QUEUE + GS_IX_MAX_HASHES) * sizeof(u64))

template <bool BM_LDS>
__global__ __launch_bounds__(GS_IX_BLOCK) void gs_index_kernel(GsIndexParams P) {
    extern __shared__ u64 lds[];
    u64 *queue = lds + (threadIdx.x >> 6) * GS_IX_QUEUE;
    int64_t *factors = reinterpret_cast<int64_t *>(lds + (GS_IX_BLOCK / 64) * GS_IX_QUEUE);
    uint32_t *lds_bm = reinterpret_cast<uint32_t *>(factors + GS_IX_MAX_HASHES);
    if (P.put)
        for (int i = threadIdx.x; i < P.n_hashes && i < GS_IX_MAX_HASHES; i += blockDim.x) factors[i] = P.factors[i];
    if (BM_LDS)
        for (int i = threadIdx.x; i < (P.n_values + 31) >> 5; i += blockDim.x) lds_bm[i] = P.requested[i];
    __syncthreads();
    auto requested = [&](int32_t v) { return (((BM_LDS ? lds_bm[v >> 5] : P.requested[v >> 5]) >> (v & 31)) & 1u) != 0; };

    const int lane = threadIdx.x & 63, q = lane & 3;
    const int64_t n_lines = P.n_rec + P.n_tab;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint32_t kmask = (uint32_t)((1ULL << P.k) - 1);
    const uint32_t vmask = (1u << P.vbits) - 1u;
    const int nh = P.n_hashes;
    uint32_t *words32 = reinterpret_cast<uint32_t *>(P.words);  // bit i = bit (i & 31) of 32-bit word i >> 5 (little endian)
    u64 wave_count = 0;
    // (the loop bound is uniform per wave: lines are whole quads, a quad never straddles a wave)
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); t0 < 4 * n_lines; t0 += stride) {
        const int64_t line = (t0 + lane) >> 2;
        const bool is_rec = line < P.n_rec;
        u64 x0, x1;
        gs_ex_load_quad(P.rec, P.tab, P.n_rec, n_lines, line, q, x0, x1);
        const int src = lane & ~3;
        const u64 w0 = __shfl(x0, src), w1 = __shfl(x1, src);
        // which of the lane's (up to six) entries are selected: bit i = record offset 6 (q - 1) + i / table slot 2 q + i
        uint32_t sel = 0;
        if (line < n_lines) {
            if (is_rec) {
                const uint32_t valid = gs_ex_rec_valid(w1, q);
                for (int i = 0; i < GS_EX_MAX_PER_LANE; i++)
                    if ((valid >> i) & 1u) {
                        const int32_t v = gs_ex_rec_value(x0, x1, i);
                        if (v < P.n_values && requested(v)) sel |= 1u << i;
                    }
            } else {
                for (int i = 0; i < 2; i++) {
                    const int32_t v = gs_ex_tab_value(i ? x1 : x0, vmask);
                    if (v >= 0 && v < P.n_values && requested(v)) sel |= 1u << i;
                }
            }
        }
        int before, total;
        gs_ex_wave_prefix(__popc(sel), lane, before, total);
        wave_count += (u64)total;
        if (!P.put || total == 0) continue;
        // the wave's selected keys, compacted into its queue (before + popc(sel) <= total <= GS_IX_QUEUE)
        for (uint32_t m = sel; m; m &= m - 1, before++) {
            const int i = __builtin_ctz(m);
            queue[before] = is_rec ? gs_ex_rec_key(w0, w1, 6 * (q - 1) + i, P.k, kmask)
                                   : gs_ex_tab_key(i ? x1 : x0, (u64)(P.tab_first + (line - P.n_rec)), P.vbits, P.bucket_bits, P.k, kmask);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (P.kind == GS_BLOOM_BLOCKED) {
            for (int p = lane; p < total; p += 64) {
                const int64_t h0 = factors[0] ^ (int64_t)queue[p];
                const u64 start = gs_absmod(h0, P.bits, P.magic, P.magic_shift);
                u64 uh = (u64)h0;
                uh ^= (uh << 32) | (uh >> 32);
                const int64_t sh = (int64_t)uh;  // (Java masks a long shift count to 6 bits; >> is arithmetic)
                const u64 m1 = (1ULL << (sh & 63)) | (1ULL << ((sh >> 6) & 63));
                const u64 m2 = (1ULL << ((sh >> 12) & 63)) | (1ULL << ((sh >> 18) & 63));
                u64 *a = P.words + start, *b = P.words + start + 1 + (uh >> 60);
                if ((*a & m1) != m1) atomicOr(a, m1);
                if ((*b & m2) != m2) atomicOr(b, m2);
            }
        } else {
            // the (key, hash) pairs of the step spread over the lanes: lane l takes pairs l, l + 64, ..; pair p = key p / nh, hash p % nh
            const int pairs = total * nh;
            for (int p = lane; p < pairs; p += 64) {
                const int j = nh == 1 ? p : (int)__umulhi((uint32_t)p, P.hash_inv);
                const int64_t key = (int64_t)queue[j], f = factors[p - j * nh];
                const int64_t h = P.kind == GS_BLOOM_XOR ? (f ^ key) : gs_murmur64(key, f);
                const u64 idx = gs_absmod(h, P.bits, P.magic, P.magic_shift);
                uint32_t *w = words32 + (uint32_t)(idx >> 5);
                const uint32_t m = 1u << (idx & 31);
                if ((*w & m) == 0) atomicOr(w, m);  // a set bit costs no atomic (a stale 0 only costs one more)
            }
        }
        __builtin_amdgcn_wave_barrier();  // the queue is rewritten by the next step
    }
    if (lane == 0 && wave_count != 0) atomicAdd(P.count, wave_count);
}

extern "C" hipError_t gs_launch_index(const GsIndexParams *P, int n_cu, hipStream_t stream) {
    const int64_t threads = 4 * (P->n_rec + P->n_tab);
    if (threads == 0) return hipSuccess;
    int64_t grid = (threads + GS_IX_BLOCK - 1) / GS_IX_BLOCK;
    const int64_t cap = (int64_t)n_cu * 8;  // grid-stride beyond ~8 workgroups per CU (the bitmap is staged once per workgroup)
    if (grid > cap) grid = cap;
    const int bm_words = (P->n_values + 31) >> 5;
    if (bm_words <= GS_IX_LDS_WORDS)
        hipLaunchKernelGGL(gs_index_kernel<true>, dim3((unsigned)grid), dim3(GS_IX_BLOCK), GS_IX_LDS_FIXED + (size_t)bm_words * sizeof(uint32_t), stream, *P);
    else
        hipLaunchKernelGGL(gs_index_kernel<false>, dim3((unsigned)grid), dim3(GS_IX_BLOCK), GS_IX_LDS_FIXED, stream, *P);
    return hipGetLastError();
}
