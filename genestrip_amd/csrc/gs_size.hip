// gs_size.hip -- a genome collection sized on the device before it is built (include/gsgpu.h, gs_dbsize_*): the two walks the
// reference makes in front of filldb,
//   fillsize   (C/goals/refseq/FillSizeGoal.java:80-105 over C/refseq/AbstractStoreFastaReader.java:87-115): k-mers with
//              duplicates, those the low-complexity gate drops (dustCounter), those that remain        gs_size_count_kernel
//   tempindex  (C/goals/refseq/FillBloomFilterGoal.java:154-195, :260-271): distinct k-mers, in total and per radix bucket
//              (RadixKMerStore.radixOf)                     retained keys -> rocPRIM radix sort -> gs_size_heads_kernel
// The counting kernel reads one byte per base and writes nothing per k-mer: counters in registers, a histogram of the
// canonical k-mer's top bits in LDS.  HBM-bound on the read (1 B per base).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "gs_build_dev.h"
#include "gs_launch.h"

#define GS_SIZE_BLOCK 256  // 4 waves: nothing here is per workgroup and step (the builder's 1024 serve its pair counter)
#define GS_SIZE_MAX_BINS 4096

// 64-bit value of lane 0 on every lane (the wave is converged where this is called)
__device__ __forceinline__ u64 gs_size_first(u64 v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((u64)hi << 32) | lo;
}

// One wave per tile of 64 consecutive base positions, the tile decode of gs_build_kmers_kernel (gs_build_dev.h): three ballot
// planes, a funnel shift per lane, the window rule of the reference.  What differs is what happens to a window:
//   total / dust / included   popcounts of ballots, summed in scalar registers over the wave's tiles: three atomics per wave
//   per_value[tag]            while the wave's tiles lie in regions of one tag the count stays in a register and leaves with one
//                             64-bit atomic when the tag changes or the wave ends: all genomes of one tax id hit one address, and
//                             a device-scope atomic is worked off at the memory side one after the other, so
//                             one atomic per tile would queue there.  A tile in which a region ends takes the per-lane path.
//   hist[canon >> shift]      32-bit LDS bins per workgroup, flushed with 64-bit global atomics at the end.  A bin cannot wrap:
//                             a workgroup adds at most one per position it walks, and the launcher gives no workgroup 2^32
//                             positions (gs_launch_size_count raises the grid for batches of 2^31 bases and more).
//   KEEP                      the canonical k-mers in [range_lo, range_hi) go behind each other into keys (one returning atomic
//                             per wave and tile), for the distinct pass
template <bool KEEP>
__global__ __launch_bounds__(GS_SIZE_BLOCK) void gs_size_count_kernel(const GsSizeParams P) {
    __shared__ uint32_t s_hist[GS_SIZE_MAX_BINS];
    for (int b = (int)threadIdx.x; b < P.hist_bins; b += GS_SIZE_BLOCK) s_hist[b] = 0;
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63);
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (wave-uniform, and known to be: scalar loads below)
    const int k = P.k;
    const uint32_t kmask = (uint32_t)((1ULL << k) - 1);
    const int64_t total = P.total, n_regions = P.n_regions;
    const int64_t n_tiles = (total + 63) >> 6;
    const int64_t n_waves = (int64_t)gridDim.x * (GS_SIZE_BLOCK / 64);
    u64 w_total = 0, w_dust = 0, w_incl = 0;  // of this wave
    int32_t cur_tag = -1;                     // the tag whose count is in cur_cnt
    u64 cur_cnt = 0;
    for (int64_t tile = (int64_t)blockIdx.x * (GS_SIZE_BLOCK / 64) + wib; tile < n_tiles; tile += n_waves) {
        const int64_t p0 = tile << 6, p = p0 + lane;  // (p0 < total)
        // bytes p0 .. p0 + 63 and p0 + 64 .. p0 + 64 + k - 2
        const uint32_t c0 = p < total ? gs_build_code(P.seq[p], P.lower) : 4u;
        const uint32_t c1 = (lane < k - 1 && p + 64 < total) ? gs_build_code(P.seq[p + 64], P.lower) : 4u;
        const u64 hi0 = __ballot((c0 >> 1) & 1u), lo0 = __ballot(c0 & 1u), bad0 = __ballot(c0 >> 2);
        const u64 hi1 = __ballot((c1 >> 1) & 1u), lo1 = __ballot(c1 & 1u), bad1 = __ballot(c1 >> 2);
        // region of the tile's first position: the last r with off[r] <= p0, one search per wave
        int64_t lo = 0, hi = n_regions;  // invariant: off[lo] <= p0 < off[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (P.off[mid] <= (u64)p0)
                lo = mid;
            else
                hi = mid;
        }
        int64_t r = lo;
        u64 r_begin = P.off[lo], r_end = P.off[lo + 1];
        const bool straddle = r_end < (u64)(p0 + 64 + k - 1) && r_end < (u64)total;  // a region ends inside the tile (wave-uniform)
        if (straddle) {  // every lane finds its own
            int64_t l2 = lo, h2 = n_regions;
            while (h2 - l2 > 1) {
                const int64_t mid = (l2 + h2) >> 1;
                if (P.off[mid] <= (u64)p)
                    l2 = mid;
                else
                    h2 = mid;
            }
            r = l2;
            r_begin = P.off[l2];
            r_end = P.off[l2 + 1];
        }
        const uint32_t wbad = gs_build_funnel(bad0, bad1, lane, kmask);
        const int64_t s_in = p - (int64_t)r_begin;
        const bool window = p < total && wbad == 0 && (u64)p + (u64)k <= r_end && (s_in + k) % P.step == 0;
        u64 key = 0;
        bool dust = false;
        if (window) {
            // planes: bit i = base p + i.  Reference encoding: base p in the top bit pair.
            const uint32_t fhi = gs_build_funnel(hi0, hi1, lane, kmask), flo = gs_build_funnel(lo0, lo1, lane, kmask);
            const uint32_t rhi = __brev(fhi) >> (32 - k), rlo = __brev(flo) >> (32 - k);
            const u64 fwd = (gs_build_spread(rhi) << 1) | gs_build_spread(rlo);
            const u64 rev = (gs_build_spread(fhi) << 1) | gs_build_spread((flo ^ kmask) & kmask);  // complement: C<->G, A<->T, reversed
            key = fwd > rev ? fwd : rev;  // CGAT.standardKMer (:145-147)
            dust = P.max_dust >= 0 && gs_build_dust(fhi, flo, k) > P.max_dust;  // isDust(): dustCounter, nothing else
        }
        const bool incl = window && !dust;
        const u64 n_incl = (u64)__popcll(__ballot(incl));
        w_total += (u64)__popcll(__ballot(window));
        w_dust += (u64)__popcll(__ballot(dust));
        w_incl += n_incl;
        if (incl) atomicAdd(&s_hist[(uint32_t)(key >> P.hist_shift)], 1u);
        if (!straddle) {
            const int32_t tag = P.tag[r];  // (r is the wave's here)
            if (tag != cur_tag) {
                if (cur_cnt && lane == 0) atomicAdd(&P.per_value[cur_tag], cur_cnt);
                cur_tag = tag;
                cur_cnt = 0;
            }
            cur_cnt += n_incl;
        } else if (incl)
            atomicAdd(&P.per_value[P.tag[r]], 1ULL);
        if (KEEP) {
            const bool keep = incl && key >= P.range_lo && key < P.range_hi;  // (gs_dbsize_set_range: another pass takes the rest)
            const u64 have = __ballot(keep);
            if (have) {
                u64 base = 0;
                if (lane == 0) base = atomicAdd(P.n_keys, (u64)__popcll(have));
                base = gs_size_first(base);
                const u64 at = base + (u64)__popcll(have & ((1ULL << lane) - 1));
                if (keep && at < P.keys_cap) P.keys[at] = key;  // (the host reserves a slot per position: the bound never bites)
            }
        }
    }
    if (lane == 0) {
        if (cur_cnt) atomicAdd(&P.per_value[cur_tag], cur_cnt);
        if (w_total) atomicAdd(&P.totals[0], w_total);
        if (w_dust) atomicAdd(&P.totals[1], w_dust);
        if (w_incl) atomicAdd(&P.totals[2], w_incl);
    }
    __syncthreads();
    for (int b = (int)threadIdx.x; b < P.hist_bins; b += GS_SIZE_BLOCK) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(&P.hist[b], (u64)c);
    }
}

// Over the ascending keys: the head of every run of equal keys is one distinct k-mer and one more in its radix bucket.  The
// bucket is the key's LOW bits, which change from one head to the next: neighbouring heads hit different addresses, so the
// bucket array takes plain global atomics and needs no private copy.  The count leaves with one atomic per wave.
__global__ __launch_bounds__(256) void gs_size_heads_kernel(const u64 *keys, int64_t n, u64 radix_mask, u64 *n_distinct, u64 *buckets) {
    uint32_t mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 key = keys[i];
        if (i == 0 || keys[i - 1] != key) {
            mine++;
            if (buckets) atomicAdd(&buckets[key & radix_mask], 1ULL);
        }
    }
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_distinct, (u64)mine);
}

static int gs_size_env(const char *name) {
    const char *s = getenv(name);
    const int v = s ? atoi(s) : 0;
    return v > 0 ? v : 0;
}

// GS_SIZE_BLOCKS_PER_CU workgroups per CU (default 8: 32 waves per CU, what the kernel's registers allow); GS_SIZE_GRID caps
// the grid outright (tests make a few thousand bases wrap the grid-stride loop with it)
extern "C" hipError_t gs_launch_size_count(const GsSizeParams *P, int n_cu, hipStream_t stream) {
    if (P->total <= 0 || P->n_regions <= 0) return hipSuccess;
    const int per_cu = gs_size_env("GS_SIZE_BLOCKS_PER_CU"), cap = gs_size_env("GS_SIZE_GRID");
    int64_t grid = (int64_t)(n_cu > 0 ? n_cu : 256) * (per_cu ? per_cu : 8);
    const int64_t tiles = (P->total + 63) >> 6, need = (tiles + GS_SIZE_BLOCK / 64 - 1) / (GS_SIZE_BLOCK / 64);
    if (grid > need) grid = need;
    if (cap && grid > cap) grid = cap;
    // the LDS bins are 32 bits wide: a workgroup walks total / grid + 256 positions at the most, below 2^32 with this floor
    const int64_t floor = (P->total >> 31) + 1;
    if (grid < floor) grid = floor;
    if (P->keys)
        hipLaunchKernelGGL(gs_size_count_kernel<true>, dim3((unsigned)grid), dim3(GS_SIZE_BLOCK), 0, stream, *P);
    else
        hipLaunchKernelGGL(gs_size_count_kernel<false>, dim3((unsigned)grid), dim3(GS_SIZE_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

// bytes of temporary storage the sort of n keys takes (no device work)
extern "C" hipError_t gs_size_sort_bytes(int64_t n, int key_bits, size_t *tmp_bytes) {
    *tmp_bytes = 0;
    if (n <= 1) return hipSuccess;
    rocprim::double_buffer<u64> dk(nullptr, nullptr);
    return rocprim::radix_sort_keys(nullptr, *tmp_bytes, dk, (size_t)n, 0, (unsigned)key_bits, nullptr);
}

// keys: n keys, sorted through keys_alt (n) and tmp (gs_size_sort_bytes); *keys_out = the buffer that holds the result
extern "C" hipError_t gs_size_sort(u64 *keys, u64 *keys_alt, int64_t n, int key_bits, void *tmp, size_t tmp_bytes, u64 **keys_out,
                                   hipStream_t stream) {
    *keys_out = keys;
    if (n <= 1) return hipSuccess;
    rocprim::double_buffer<u64> dk(keys, keys_alt);
    const hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, dk, (size_t)n, 0, (unsigned)key_bits, stream);
    *keys_out = dk.current();
    return e;
}

extern "C" hipError_t gs_launch_size_heads(const u64 *keys, int64_t n, int radix_bits, u64 *n_distinct, u64 *buckets, int n_cu,
                                           hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    int64_t grid = (n + 255) / 256;
    const int64_t most = (int64_t)(n_cu > 0 ? n_cu : 256) * 8;
    if (grid > most) grid = most;
    hipLaunchKernelGGL(gs_size_heads_kernel, dim3((unsigned)grid), dim3(256), 0, stream, keys, n, ((u64)1 << radix_bits) - 1, n_distinct,
                       radix_bits > 0 ? buckets : nullptr);
    return hipGetLastError();
}
