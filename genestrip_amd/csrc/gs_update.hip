// gs_update.hip -- a finished store updated in batches (include/gsgpu.h, gs_dbupdate_*): the compute core of the reference's
// updatedb stage (DBGoal.MyFastaReader, C/goals/refseq/DBGoal.java:233-311) in its own streaming shape.  The store's k-mers
// (ascending) and values stay on the device; regions stream past them slice by slice:
//   every k-mer of every region of a slice -> (canonical k-mer, region) pairs     gs_build_kmers_kernel (gs_build.hip, unchanged)
//   per pair: directory bucket -> short search in the k-mer array -> on a hit
//   value := LCA(value, node of the region)                                        gs_upd_lookup_kernel
// LCA is associative, commutative and idempotent, so pairs, slices and batches may land in any order: nothing is sorted and
// nothing but the store outlives a slice.
//
// The directory (built once per handle): bucket b holds the stored k-mers i with gs_upd_bucket(k-mer) == b, dir[b] = the first
// of them.  Canonical k-mers are the larger of two strands, so their density grows linearly over the key space
// (P(x <= t) ~ (t / 4^k)^2, genestrip_amd.binding.kmer_ranges); the bucket number is the SQUARE of the key's top 32 bits, which
// gives buckets of about equal fill.  A pair costs one directory line plus the bucket's keys (one or two lines); a miss stops
// there and never touches a value.  For small k the directory has at most 4^k buckets and the search inside a bucket is binary.
//
// Values only ever move towards the root.  A lane that reads a stale value (the L2 of another XCD) either sees that nothing
// changes -- then the region's node lies below the stale value, hence below the current one -- or its compare-and-swap fails
// and hands it the current value.  The atomics are ordinary vector atomics at device scope.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_build_dev.h"
#include "gs_launch.h"

#define GS_UPD_BLOCK 256
#define GS_UPD_LINEAR 4  // buckets up to this many k-mers are walked, longer ones halved first

// key < 4^k.  Non-decreasing in key.
__device__ __forceinline__ uint32_t gs_upd_bucket(u64 key, int k, int dir_bits) {
    const u64 u = 2 * k >= 32 ? key >> (2 * k - 32) : key << (32 - 2 * k);
    return (uint32_t)((u * u) >> (64 - dir_bits));
}

// flag |= 1: a k-mer outside [0, 4^k) or not above its predecessor; |= 2: a value index outside [0, n_values)
__global__ __launch_bounds__(GS_UPD_BLOCK) void gs_upd_check_kernel(const u64 *keys, const int32_t *vals, int64_t m, int k, int32_t n_values,
                                                                    uint32_t *flag) {
    const u64 top = 1ULL << (2 * k);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 key = keys[i];
        uint32_t bad = (key >= top || (i > 0 && keys[i - 1] >= key)) ? 1u : 0u;
        const int32_t v = vals[i];
        if (v < 0 || v >= n_values) bad |= 2u;
        if (bad) atomicOr(flag, bad);
    }
}

template <typename OFF>
__global__ __launch_bounds__(GS_UPD_BLOCK) void gs_upd_dir_fill_kernel(OFF *dir, int64_t n, OFF value) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dir[i] = value;
}

// dir is preset to m; the first k-mer of every bucket writes the starts of its bucket and of the empty ones in front of it
template <typename OFF>
__global__ __launch_bounds__(GS_UPD_BLOCK) void gs_upd_dir_kernel(const u64 *keys, int64_t m, int k, int dir_bits, OFF *dir) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = (int64_t)gs_upd_bucket(keys[i], k, dir_bits);
        const int64_t pb = i > 0 ? (int64_t)gs_upd_bucket(keys[i - 1], k, dir_bits) : -1;
        for (int64_t x = pb + 1; x <= b; x++) dir[x] = (OFF)i;
    }
}

// One lane per pair.  Found: the value moves to LCA(value, node) unless it is there already (the common case once the values
// have converged: no write) or has no tree node (DBGoal.java:246-251: lastLCA = lcaNode != null ? ... : oldValue).
template <typename OFF>
__global__ __launch_bounds__(GS_UPD_BLOCK) void gs_upd_lookup_kernel(GsUpdateParams P) {
    const OFF *dir = (const OFF *)P.dir;
    const int64_t n = (int64_t)*P.n_pairs;
    uint32_t found = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const u64 key = P.keys[i];
        const uint32_t b = gs_upd_bucket(key, P.k, P.dir_bits);
        int64_t lo = (int64_t)dir[b], hi = (int64_t)dir[b + 1];  // the k-mer, if stored, lies in [lo, hi)
        while (hi - lo > GS_UPD_LINEAR) {
            const int64_t mid = (lo + hi) >> 1;
            if (P.skeys[mid] <= key)
                lo = mid;
            else
                hi = mid;
        }
        int64_t at = -1;
        for (int64_t j = lo; j < hi; j++) {
            const u64 kk = P.skeys[j];
            if (kk == key) at = j;
            if (kk >= key) break;
        }
        if (at < 0) continue;
        found++;
        const int32_t node = P.node_of_region[P.region[i]];
        int32_t v = P.svals[at];
        while (v != node && P.parent[v] != -2) {
            const int32_t l = gs_build_lca(P.parent, P.depth, v, node);
            if (l == v) break;
            const int32_t old = atomicCAS(&P.svals[at], v, l);
            if (old == v) break;
            v = old;  // another lane moved it: towards the root, so the loop ends
        }
    }
    for (int d = 32; d > 0; d >>= 1) found += (uint32_t)__shfl_down((int)found, d);
    if ((threadIdx.x & 63) == 0 && found) atomicAdd(&P.stats[1], (u64)found);
    if (blockIdx.x == 0 && threadIdx.x == 0 && n) atomicAdd(&P.stats[0], (u64)n);
}

__global__ __launch_bounds__(GS_UPD_BLOCK) void gs_upd_moved_kernel(const int32_t *vals, const int32_t *vals0, int64_t m, u64 *count) {
    uint32_t c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) c += vals[i] != vals0[i];
    for (int d = 32; d > 0; d >>= 1) c += (uint32_t)__shfl_down((int)c, d);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (u64)c);
}

static unsigned gs_upd_grid(int64_t n, int n_cu) {
    int64_t g = (n + GS_UPD_BLOCK - 1) / GS_UPD_BLOCK;
    const int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 256) * 16;  // (a wave counts its hits in 32 bits: far below 2^32 pairs each)
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

extern "C" hipError_t gs_launch_update_check(const u64 *keys, const int32_t *vals, int64_t m, int k, int32_t n_values, uint32_t *flag, int n_cu,
                                             hipStream_t stream) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_upd_check_kernel, dim3(gs_upd_grid(m, n_cu)), dim3(GS_UPD_BLOCK), 0, stream, keys, vals, m, k, n_values, flag);
    return hipGetLastError();
}

// dir: (1 << dir_bits) + 1 entries of 4 (wide: 8) bytes
extern "C" hipError_t gs_launch_update_dir(const u64 *keys, int64_t m, int k, int dir_bits, int wide, void *dir, int n_cu, hipStream_t stream) {
    const int64_t n_dir = ((int64_t)1 << dir_bits) + 1;
    if (wide)
        hipLaunchKernelGGL(gs_upd_dir_fill_kernel<u64>, dim3(gs_upd_grid(n_dir, n_cu)), dim3(GS_UPD_BLOCK), 0, stream, (u64 *)dir, n_dir, (u64)m);
    else
        hipLaunchKernelGGL(gs_upd_dir_fill_kernel<uint32_t>, dim3(gs_upd_grid(n_dir, n_cu)), dim3(GS_UPD_BLOCK), 0, stream, (uint32_t *)dir, n_dir,
                           (uint32_t)m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || m <= 0) return e;
    if (wide)
        hipLaunchKernelGGL(gs_upd_dir_kernel<u64>, dim3(gs_upd_grid(m, n_cu)), dim3(GS_UPD_BLOCK), 0, stream, keys, m, k, dir_bits, (u64 *)dir);
    else
        hipLaunchKernelGGL(gs_upd_dir_kernel<uint32_t>, dim3(gs_upd_grid(m, n_cu)), dim3(GS_UPD_BLOCK), 0, stream, keys, m, k, dir_bits, (uint32_t *)dir);
    return hipGetLastError();
}

// max_pairs: an upper bound of *P->n_pairs known to the host (the bases of the slice)
extern "C" hipError_t gs_launch_update_lookup(const GsUpdateParams *P, int64_t max_pairs, int n_cu, hipStream_t stream) {
    if (max_pairs <= 0) return hipSuccess;  // (an empty store still counts its pairs: every bucket is empty)
    if (P->wide)
        hipLaunchKernelGGL(gs_upd_lookup_kernel<u64>, dim3(gs_upd_grid(max_pairs, n_cu)), dim3(GS_UPD_BLOCK), 0, stream, *P);
    else
        hipLaunchKernelGGL(gs_upd_lookup_kernel<uint32_t>, dim3(gs_upd_grid(max_pairs, n_cu)), dim3(GS_UPD_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_update_moved(const int32_t *vals, const int32_t *vals0, int64_t m, u64 *count, int n_cu, hipStream_t stream) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_upd_moved_kernel, dim3(gs_upd_grid(m, n_cu)), dim3(GS_UPD_BLOCK), 0, stream, vals, vals0, m, count);
    return hipGetLastError();
}
