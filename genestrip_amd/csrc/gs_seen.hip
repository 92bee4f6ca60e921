// gs_seen.hip -- sweeps over the seen bits that the match kernels leave in a store (table slots and super-k-mer records): unique
// k-mers per value, the compact bitmap, clearing, and the OR of the bitmaps of several runs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gs_launch.h"
#include "gs_layout.h"
#include "gs_params.h"
#include "gs_wave.h"

// ---------------------------------------------------------------------------------------------------
// unique k-mers per value: scan the bitmap, look the set slots up in the table
// (KMerUniqueCounterBits.getUniqueKmerCounts, C/store/KMerUniqueCounterBits.java:146-163)
// ---------------------------------------------------------------------------------------------------
#define GS_UNIQ_LDS 8192  // value indices whose unique counters are privatised per workgroup
__global__ __launch_bounds__(256) void gs_unique_count_kernel(const u64 *table, const uint32_t *bitmap, int64_t n_slots,
                                                             uint32_t vbits, int32_t n_values, u64 *unique) {
    __shared__ unsigned int s_cnt[GS_UNIQ_LDS];
    const bool lds = n_values <= GS_UNIQ_LDS;
    if (lds) {
        for (int i = threadIdx.x; i < n_values; i += blockDim.x) s_cnt[i] = 0;
        __syncthreads();
    }
    const u64 vmask = (1ULL << vbits) - 1;
    const int64_t n_words = (n_slots + 31) / 32;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * blockDim.x) {
        uint32_t bits = bitmap[w];
        while (bits) {
            const int b = __builtin_ctz(bits);
            bits &= bits - 1;
            const u64 s = table[w * 32 + b];
            const int vi = (int)((s >> 1) & vmask) - 1;
            if (vi >= 0) {
                if (lds)
                    atomicAdd(&s_cnt[vi], 1u);
                else
                    atomicAdd(&unique[vi], 1ULL);
            }
        }
    }
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_values; i += blockDim.x)
            if (s_cnt[i]) atomicAdd(&unique[i], (u64)s_cnt[i]);
    }
}

// seen bits of the slots -> compact bitmap (bit i = slot i); one wave per 64 slots
__global__ __launch_bounds__(256) void gs_bitmap_extract_kernel(const u64 *table, int64_t n_slots, uint32_t *bitmap) {
    const int lane = gs_lane();
    for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63LL; base < n_slots;
         base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        const u64 m = __ballot(i < n_slots && (table[i] & 1ULL));
        if (lane == 0) bitmap[base >> 5] = (uint32_t)m;
        if (lane == 1 && base + 32 < n_slots) bitmap[(base >> 5) + 1] = (uint32_t)(m >> 32);
    }
}

// ---- the same sweeps over the super-k-mer records: the compact bitmap holds one 32-bit word per record bucket
// (bit j = seen bit of offset j) behind the words of the table slots.  The sweeps stream the record lines with 16-byte
// loads of consecutive threads (a thread per line and 8 bytes of it costs one 64-byte request per lane: ~4x slower on a
// 9 GB table); thread 4 b holds words 0 and 1 of bucket b.
__global__ __launch_bounds__(256) void gs_rec_bitmap_extract_kernel(const u64 *rec, int64_t n_rec, uint32_t *bitmap_rec) {
    const int64_t n = n_rec * (GS_REC_WORDS / 2);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const gs_u64x2 v = reinterpret_cast<const gs_u64x2 *>(rec)[t];
        if ((t & 3) == 0) bitmap_rec[t >> 2] = (uint32_t)(v.x >> GS_REC_WIN_BITS);
    }
}

// the three value fields of value word `w` whose bits in `bt3` (seen & valid of their offsets) are set: equal neighbouring values
// in one atomic (the k-mers of a word usually carry the same value index), into cnt[] (LDS) or unique[] (cnt == nullptr)
static __device__ __forceinline__ void gs_count_value_word(u64 w, uint32_t bt3, int32_t n_values, unsigned int *cnt, u64 *unique) {
    int v[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int vi = (int)((w >> (GS_REC_VAL_BITS * i)) & (GS_REC_MAX_VALUES - 1));
        v[i] = (((bt3 >> i) & 1u) && vi < n_values) ? vi : -1;
        c[i] = 1;
    }
    if (v[1] >= 0 && v[1] == v[0]) {
        c[0]++;
        v[1] = -1;
    }
    if (v[2] >= 0 && v[2] == v[0]) {
        c[0]++;
        v[2] = -1;
    } else if (v[2] >= 0 && v[2] == v[1]) {
        c[1]++;
        v[2] = -1;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (v[i] >= 0) {
            if (cnt)
                atomicAdd(&cnt[v[i]], (unsigned int)c[i]);
            else
                atomicAdd(&unique[v[i]], (u64)c[i]);
        }
    }
}

// 8 lanes per bucket: lane g holds word g of the line (one coalesced 64-byte request per bucket, only for buckets with a
// seen bit); lanes 2..7 look at the three value fields of their word
__global__ __launch_bounds__(256) void gs_rec_unique_count_kernel(const u64 *rec, const uint32_t *bitmap_rec, int64_t n_rec,
                                                                 int32_t n_values, u64 *unique) {
    __shared__ unsigned int s_cnt[GS_UNIQ_LDS];
    const bool lds = n_values <= GS_UNIQ_LDS;
    if (lds) {
        for (int i = threadIdx.x; i < n_values; i += blockDim.x) s_cnt[i] = 0;
        __syncthreads();
    }
    const int g = (int)(threadIdx.x & 7);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> 3;
    // eight lanes per bucket; four buckets per group and iteration with their loads in flight together (the loop is bound by
    // the latency of bitmap word -> record line, not by bytes)
    for (int64_t b0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; b0 < n_rec; b0 += 4 * groups) {
        uint32_t bits[4];
        u64 w[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t bb = b0 + u * groups;
            bits[u] = bb < n_rec ? bitmap_rec[bb] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) w[u] = bits[u] ? rec[(b0 + u * groups) * GS_REC_WORDS + g] : 0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const u64 w1 = __shfl(w[u], 1, 8);
            const uint32_t bt = bits[u] & (uint32_t)(w1 >> GS_REC_WIN_BITS);  // only offsets that hold a k-mer (a merged bitmap comes from other ranks)
            if (g >= 2 && bt) {
                gs_count_value_word(w[u], (bt >> (3 * (g - 2))) & 7u, n_values, lds ? s_cnt : nullptr, unique);
            }
        }
    }
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_values; i += blockDim.x)
            if (s_cnt[i]) atomicAdd(&unique[i], (u64)s_cnt[i]);
    }
}

// ---- extract and count in ONE pass over the store (gs_match_finish on the run's own seen bits): the extract sweep already
// loads every byte of every line, so the value words of a line with a seen bit are in registers when its bitmap word is
// written -- no second, dependent pass from the bitmap back to the lines.
// LDS counters in several copies (a lane takes copy lane % copies): the k-mers of a small taxonomy would otherwise meet on a
// few LDS words, and atomics of one wave on one word go one after the other.  The stride is odd, so that the copies of one
// value index lie in different banks.
struct GsUniqLds {
    int copies, stride;  // copies: a power of two
};
static __device__ __forceinline__ GsUniqLds gs_uniq_lds_shape(int32_t n_values) {
    GsUniqLds s = {1, n_values};
    if (2 * (n_values | 1) <= GS_UNIQ_LDS) {
        s.stride = n_values | 1;
        while (s.copies < 32 && 2 * s.copies * s.stride <= GS_UNIQ_LDS) s.copies *= 2;
    }
    return s;
}

#define GS_SWEEP_UNROLL 4    // 16-byte loads a thread has in flight
#define GS_SWEEP_BLOCK 1024  // ... and GS_SWEEP_GRID workgroups of so many threads: see gs_launch_seen_sweep
#define GS_SWEEP_GRID 512
// Record lines first (four threads per line, thread 4 b + j holds words 2 j and 2 j + 1 of bucket b), then the table slots (one
// wave per 64 slots) in the same grid; bitmap / bitmap_rec are written whole, as by the two extract kernels.
__global__ __launch_bounds__(GS_SWEEP_BLOCK) void gs_seen_sweep_kernel(const u64 *table, int64_t n_slots, uint32_t vbits, const u64 *rec, int64_t n_rec,
                                                           uint32_t *bitmap, uint32_t *bitmap_rec, int32_t n_values, u64 *unique) {
    __shared__ unsigned int s_cnt[GS_UNIQ_LDS];
    const bool lds = n_values <= GS_UNIQ_LDS;
    const GsUniqLds shape = gs_uniq_lds_shape(n_values);
    if (lds) {
        for (int i = threadIdx.x; i < shape.copies * shape.stride; i += blockDim.x) s_cnt[i] = 0;
        __syncthreads();
    }
    unsigned int *cnt = lds ? s_cnt + (threadIdx.x & (shape.copies - 1)) * shape.stride : nullptr;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;  // (a multiple of 4: the four threads of a line stay together)
    const int64_t n = n_rec * (GS_REC_WORDS / 2);
    const int j = (int)(threadIdx.x & 3);
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t0 < n; t0 += GS_SWEEP_UNROLL * stride) {
        gs_u64x2 v[GS_SWEEP_UNROLL];
#pragma unroll
        for (int u = 0; u < GS_SWEEP_UNROLL; u++) {
            const int64_t t = t0 + u * stride;
            v[u] = t < n ? reinterpret_cast<const gs_u64x2 *>(rec)[t] : gs_u64x2{0, 0};
        }
#pragma unroll
        for (int u = 0; u < GS_SWEEP_UNROLL; u++) {
            const int64_t t = t0 + u * stride;
            const uint32_t seen = (uint32_t)(v[u].x >> GS_REC_WIN_BITS);
            if (j == 0 && t < n) bitmap_rec[t >> 2] = seen;
            // seen & valid of the line's offsets, from the thread that holds w0 / w1, to the three that hold the value words
            const uint32_t bt = (uint32_t)__shfl((int)(seen & (uint32_t)(v[u].y >> GS_REC_WIN_BITS)), 0, 4);
            if (j != 0 && bt) {  // value word g = 2 j + h holds the offsets 3 (g - 2) ..
                const uint32_t b6 = bt >> (6 * (j - 1));
                if (b6 & 7u) gs_count_value_word(v[u].x, b6 & 7u, n_values, cnt, unique);
                if ((b6 >> 3) & 7u) gs_count_value_word(v[u].y, (b6 >> 3) & 7u, n_values, cnt, unique);
            }
        }
    }
    const u64 vmask = (1ULL << vbits) - 1;
    const int lane = gs_lane();
    for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63LL; base < n_slots; base += stride) {
        const int64_t i = base + lane;
        const u64 s = i < n_slots ? table[i] : 0;
        const u64 m = __ballot((s & 1ULL) != 0);
        if (lane == 0) bitmap[base >> 5] = (uint32_t)m;
        if (lane == 1 && base + 32 < n_slots) bitmap[(base >> 5) + 1] = (uint32_t)(m >> 32);
        const int vi = (int)((s >> 1) & vmask) - 1;
        if ((s & 1ULL) && vi >= 0 && vi < n_values) {
            if (lds)
                atomicAdd(&cnt[vi], 1u);
            else
                atomicAdd(&unique[vi], 1ULL);
        }
    }
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_values; i += blockDim.x) {
            unsigned int a = 0;
            for (int c = 0; c < shape.copies; c++) a += s_cnt[c * shape.stride + i];
            if (a) atomicAdd(&unique[i], (u64)a);
        }
    }
}

// the seen bits of the record lines and of the table slots, cleared in one launch
__global__ __launch_bounds__(256) void gs_clear_seen_kernel(u64 *table, int64_t n_slots, u64 *rec, int64_t n_rec) {
    const u64 M47 = (1ULL << GS_REC_WIN_BITS) - 1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n = n_rec * (GS_REC_WORDS / 2);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const gs_u64x2 v = reinterpret_cast<const gs_u64x2 *>(rec)[t];
        if ((t & 3) == 0 && (v.x >> GS_REC_WIN_BITS)) rec[2 * t] = v.x & M47;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const u64 s = table[i];
        if (s & 1ULL) table[i] = s & ~1ULL;
    }
}

__global__ __launch_bounds__(256) void gs_bitmap_or_kernel(uint32_t *dst, const uint32_t *parts, int64_t n_words, int64_t n_parts) {
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * blockDim.x) {
        uint32_t v = dst[w];
        for (int64_t p = 0; p < n_parts; p++) v |= parts[p * n_words + w];
        dst[w] = v;
    }
}

// the compact bitmap: (n_slots + 31) / 32 words for the table slots, then one word per record bucket (rec may be NULL)
extern "C" hipError_t gs_launch_unique_count(const u64 *table, const uint32_t *bitmap, int64_t n_slots, uint32_t vbits,
                                              int32_t n_values, u64 *unique, const u64 *rec, int64_t n_rec, hipStream_t stream) {
    int64_t n_words = (n_slots + 31) / 32;
    int grid = (int)((n_words + 255) / 256);
    if (grid > 4096) grid = 4096;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(gs_unique_count_kernel, dim3(grid), dim3(256), 0, stream, table, bitmap, n_slots, vbits, n_values, unique);
    if (rec != nullptr && n_rec > 0) {
        grid = (int)std::min<int64_t>((n_rec * 8 + 255) / 256, 2048);
        hipLaunchKernelGGL(gs_rec_unique_count_kernel, dim3(grid), dim3(256), 0, stream, rec, bitmap + n_words, n_rec, n_values, unique);
    }
    return hipGetLastError();
}

// one stripe of a striped store: `rec` = the stripe's lines, `bitmap_rec` = the bitmap words of ITS buckets
extern "C" hipError_t gs_launch_rec_unique_count(const u64 *rec, const uint32_t *bitmap_rec, int64_t n_rec, int32_t n_values,
                                                  u64 *unique, hipStream_t stream) {
    if (n_rec <= 0) return hipSuccess;
    const int grid = (int)std::min<int64_t>((n_rec * 8 + 255) / 256, 2048);
    hipLaunchKernelGGL(gs_rec_unique_count_kernel, dim3(grid), dim3(256), 0, stream, rec, bitmap_rec, n_rec, n_values, unique);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_bitmap_extract(const u64 *table, int64_t n_slots, uint32_t *bitmap, const u64 *rec, int64_t n_rec,
                                                hipStream_t stream) {
    hipLaunchKernelGGL(gs_bitmap_extract_kernel, dim3(4096), dim3(256), 0, stream, table, n_slots, bitmap);
    if (rec != nullptr && n_rec > 0)
        hipLaunchKernelGGL(gs_rec_bitmap_extract_kernel, dim3((int)std::min<int64_t>((n_rec * 4 + 255) / 256, 8192)), dim3(256), 0, stream,
                           rec, n_rec, bitmap + (n_slots + 31) / 32);
    return hipGetLastError();
}

// gs_launch_bitmap_extract and gs_launch_unique_count of the store's own seen bits in one pass; `unique` must be zero
extern "C" hipError_t gs_launch_seen_sweep(const u64 *table, int64_t n_slots, uint32_t vbits, const u64 *rec, int64_t n_rec, uint32_t *bitmap,
                                            int32_t n_values, u64 *unique, hipStream_t stream) {
    if (rec == nullptr) n_rec = 0;
    // Few, large workgroups: every one of them ends with an atomic per value index it has met, all on the same few cache lines,
    // which take them one after the other (~1.1 ns each on MI355X, 64 MiB of records, 20 values: 1 024 workgroups of 256
    // threads 34.1 us, 512 of 1 024 threads 21.0 us, 256 of them 23.0 us -- the extract sweep alone 11.4 us)
    const int64_t items = std::max<int64_t>((n_rec * (GS_REC_WORDS / 2) + GS_SWEEP_UNROLL - 1) / GS_SWEEP_UNROLL, n_slots);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((items + GS_SWEEP_BLOCK - 1) / GS_SWEEP_BLOCK, GS_SWEEP_GRID));
    hipLaunchKernelGGL(gs_seen_sweep_kernel, dim3(grid), dim3(GS_SWEEP_BLOCK), 0, stream, table, n_slots, vbits, rec, n_rec, bitmap,
                       bitmap + (n_slots + 31) / 32, n_values, unique);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_clear_seen(u64 *table, int64_t n_slots, u64 *rec, int64_t n_rec, hipStream_t stream) {
    if (rec == nullptr) n_rec = 0;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((std::max<int64_t>(n_rec * 4, n_slots) + 255) / 256, 8192));
    hipLaunchKernelGGL(gs_clear_seen_kernel, dim3(grid), dim3(256), 0, stream, table, n_slots, rec, n_rec);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_bitmap_or(uint32_t *dst, const uint32_t *parts, int64_t n_words, int64_t n_parts,
                                           hipStream_t stream) {
    int grid = (int)((n_words + 255) / 256);
    if (grid > 4096) grid = 4096;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(gs_bitmap_or_kernel, dim3(grid), dim3(256), 0, stream, dst, parts, n_words, n_parts);
    return hipGetLastError();
}
