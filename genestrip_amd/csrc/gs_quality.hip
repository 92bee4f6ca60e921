// gs_quality.hip -- store quality against its source genomes (include/gsgpu.h, gs_dbquality_*): the compute core of the
// reference's dbqualcounts goal (ft/.../finertree/goals/DBQualityCountsGoal.java: MyFastaReader.handleStore :250-289).  The
// reference walks every genome again, looks every k-mer up in the finished store by binary search and removes duplicate
// (k-mer, leaf) pairs with one synchronized Bloom filter.  Here, in the manner of gs_build.hip:
//   every k-mer of every genome region -> (canonical k-mer, region) pairs        gs_build_kmers_kernel (gs_build.hip, unchanged)
//   region -> the region's leaf value index                                      gs_quality_tag_kernel
//   pairs sorted by (k-mer, leaf)                                                two stable radix sorts: leaf bits, then 2k key bits
//   distinct pairs joined with the store in ascending k-mer order, classified
//   by the store's tin / tout arrays and counted per leaf                        gs_quality_join_kernel
// Both sides of the join are sorted, so the pairs of a tile meet one narrow window of the store: two searches per tile find
// it, the window goes to LDS once and every pair searches there.  Integer work, HBM-bound like the builder.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "gs_launch.h"

#define GS_QUAL_BLOCK 256
#define GS_QUAL_ITEMS 4
#define GS_QUAL_TILE (GS_QUAL_BLOCK * GS_QUAL_ITEMS)
#define GS_QUAL_WINDOW 2048       // store keys of a tile held in LDS (16 KiB); wider windows are searched in global memory
#define GS_QUAL_LDS_VALUES 2048   // per-workgroup count rows in LDS up to this many values (32 KiB), global atomics beyond

// pairs [0, n): the region number the k-mer kernel wrote -> that region's leaf
__global__ __launch_bounds__(256) void gs_quality_tag_kernel(uint32_t *vals, int64_t n, const uint32_t *leaf_of_region, int64_t n_regions) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = vals[i];
        if ((int64_t)r < n_regions) vals[i] = leaf_of_region[r];
    }
}

// Pairs of one wave that count: equal leaves are added up in the wave first (a collection dominated by one taxon puts most
// pairs of a tile on ONE leaf), one lane per distinct leaf then adds to the row; after 4 leaves the rest go one by one.
__device__ __forceinline__ void gs_quality_count(bool act, bool tp, uint32_t lf, u64 *cnt) {
    const int lane = (int)(threadIdx.x & 63);
    u64 todo = __ballot(act);
    const u64 tpm = __ballot(act && tp);
    for (int round = 0; round < 4 && todo; round++) {
        const int l = __ffsll((long long)todo) - 1;
        const uint32_t lead = (uint32_t)__shfl((int)lf, l);
        const u64 same = __ballot(act && lf == lead);
        if (lane == l) {
            atomicAdd(&cnt[2 * (size_t)lead + 1], (u64)__popcll(same));
            const u64 t = (u64)__popcll(same & tpm);
            if (t) atomicAdd(&cnt[2 * (size_t)lead], t);
        }
        todo &= ~same;
    }
    if ((todo >> lane) & 1ULL) {
        atomicAdd(&cnt[2 * (size_t)lf + 1], 1ULL);
        if (tp) atomicAdd(&cnt[2 * (size_t)lf], 1ULL);
    }
}

// One workgroup per tile of GS_QUAL_TILE consecutive pairs.  The head of every run of equal (k-mer, leaf) is the distinct pair
// (the reference's Bloom filter at fpp -> 0); it counts for tp+fn when its k-mer is stored and for tp when the stored value's
// node is the leaf or one of its ancestors (tin[v] <= tin[leaf] < tout[v]).  LDS_ROWS: the count rows live in LDS and are
// flushed once per workgroup.
template <bool LDS_ROWS>
__global__ __launch_bounds__(GS_QUAL_BLOCK) void gs_quality_join_kernel(GsQualityParams P) {
    __shared__ u64 s_win[GS_QUAL_WINDOW];
    __shared__ u64 s_cnt[LDS_ROWS ? 2 * GS_QUAL_LDS_VALUES : 1];
    __shared__ int64_t s_lo, s_hi;
    const int tid = (int)threadIdx.x;
    const uint32_t nv = (uint32_t)P.n_values;
    if (LDS_ROWS) {
        for (uint32_t i = (uint32_t)tid; i < 2 * nv; i += GS_QUAL_BLOCK) s_cnt[i] = 0;
        __syncthreads();
    }
    u64 *cnt = LDS_ROWS ? s_cnt : P.counts;
    uint32_t my_heads = 0, my_found = 0;
    const int64_t n_tiles = (P.n + GS_QUAL_TILE - 1) / GS_QUAL_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * GS_QUAL_TILE;
        const int64_t end = base + GS_QUAL_TILE < P.n ? base + GS_QUAL_TILE : P.n;
        // the store window of the tile: [first key >= the tile's first k-mer, first key > its last k-mer)
        if (tid == 0 || tid == 64) {
            const u64 want = tid == 0 ? P.keys[base] : P.keys[end - 1];
            int64_t a = 0, b = P.m;
            while (a < b) {
                const int64_t mid = (a + b) >> 1;
                const u64 kk = P.skeys[mid];
                if (tid == 0 ? kk < want : kk <= want)
                    a = mid + 1;
                else
                    b = mid;
            }
            if (tid == 0)
                s_lo = a;
            else
                s_hi = a;
        }
        __syncthreads();
        const int64_t lo = s_lo, W = s_hi - s_lo;
        const bool in_lds = W <= GS_QUAL_WINDOW;
        if (in_lds)
            for (int64_t i = tid; i < W; i += GS_QUAL_BLOCK) s_win[i] = P.skeys[lo + i];
        __syncthreads();
        for (int j = 0; j < GS_QUAL_ITEMS; j++) {
            const int64_t i = base + (int64_t)j * GS_QUAL_BLOCK + tid;
            bool act = false, tp = false;
            uint32_t lf = 0;
            if (i < end) {
                const u64 key = P.keys[i];
                lf = P.leaf[i];
                const bool head = i == 0 || P.keys[i - 1] != key || P.leaf[i - 1] != lf;
                if (head && lf < nv) {
                    my_heads++;
                    int64_t a = 0, b = W;
                    while (a < b) {
                        const int64_t mid = (a + b) >> 1;
                        const u64 kk = in_lds ? s_win[mid] : P.skeys[lo + mid];
                        if (kk < key)
                            a = mid + 1;
                        else
                            b = mid;
                    }
                    if (a < W && (in_lds ? s_win[a] : P.skeys[lo + a]) == key) {
                        const uint32_t v = P.svals[lo + a];
                        if (v < nv) {  // (the decoded store only holds values with a tree node)
                            act = true;
                            my_found++;
                            const int32_t tl = P.tin[lf];
                            tp = P.tin[v] <= tl && tl < P.tout[v];
                        }
                    }
                }
            }
            gs_quality_count(act, tp, lf, cnt);
        }
        __syncthreads();  // (s_win / s_lo / s_hi are rewritten by the next tile)
    }
    if (LDS_ROWS) {
        __syncthreads();
        for (uint32_t i = (uint32_t)tid; i < 2 * nv; i += GS_QUAL_BLOCK)
            if (s_cnt[i]) atomicAdd(&P.counts[i], s_cnt[i]);
    }
    for (int d = 32; d > 0; d >>= 1) {
        my_heads += (uint32_t)__shfl_down((int)my_heads, d);
        my_found += (uint32_t)__shfl_down((int)my_found, d);
    }
    if ((tid & 63) == 0) {
        if (my_heads) atomicAdd(&P.stats[0], (u64)my_heads);
        if (my_found) atomicAdd(&P.stats[1], (u64)my_found);
    }
}

extern "C" hipError_t gs_launch_quality_tag(uint32_t *vals, int64_t n, const uint32_t *leaf_of_region, int64_t n_regions, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    int64_t g = (n + 255) / 256;
    if (g > 65536) g = 65536;
    hipLaunchKernelGGL(gs_quality_tag_kernel, dim3((unsigned)g), dim3(256), 0, stream, vals, n, leaf_of_region, n_regions);
    return hipGetLastError();
}

// the first of the two stable sorts: pairs by leaf (`bits` low bits).  Sorted in place through the alternate buffers; returns
// the buffers the sorted pairs ended up in.
extern "C" hipError_t gs_quality_sort_leaf(uint32_t *leaf, uint32_t *leaf_alt, u64 *keys, u64 *keys_alt, int64_t n, int bits, uint32_t **leaf_out,
                                           u64 **keys_out, hipStream_t stream) {
    *leaf_out = leaf;
    *keys_out = keys;
    if (n <= 1 || bits <= 0) return hipSuccess;
    rocprim::double_buffer<uint32_t> dl(leaf, leaf_alt);
    rocprim::double_buffer<u64> dk(keys, keys_alt);
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, dl, dk, (size_t)n, 0, (unsigned)bits, stream);
    if (e != hipSuccess) return e;
    void *tmp = nullptr;
    e = hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 1);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(tmp, tmp_bytes, dl, dk, (size_t)n, 0, (unsigned)bits, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    hipFree(tmp);
    *leaf_out = dl.current();
    *keys_out = dk.current();
    return e;
}

extern "C" int gs_quality_lds_values(void) { return GS_QUAL_LDS_VALUES; }

extern "C" hipError_t gs_launch_quality_join(const GsQualityParams *P, int n_cu, hipStream_t stream) {
    if (P->n <= 0) return hipSuccess;
    int64_t g = (P->n + GS_QUAL_TILE - 1) / GS_QUAL_TILE;
    const int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 256) * 4;
    if (g > cap) g = cap;
    // (a workgroup counts its heads in 32 bits: at most n / g + one tile pairs each)
    if (P->n_values <= GS_QUAL_LDS_VALUES)
        hipLaunchKernelGGL(gs_quality_join_kernel<true>, dim3((unsigned)g), dim3(GS_QUAL_BLOCK), 0, stream, *P);
    else
        hipLaunchKernelGGL(gs_quality_join_kernel<false>, dim3((unsigned)g), dim3(GS_QUAL_BLOCK), 0, stream, *P);
    return hipGetLastError();
}
