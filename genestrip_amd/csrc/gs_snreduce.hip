// gs_snreduce.hip -- the records that the FIXED loop of gs_match_kernel (counters in LDS) wrote for its reads (GsSnRec, gs_snrec.h)
// into the run's counters and per-read outputs.  gs_sn_reduce_kernel, ONE LANE PER RECORD: contigs, classification, flags and the
// row of a read of one tax id are gs_sn_row; a read without a hit gets its outputs; a read that left as a row of node codes is
// listed for gs_sn_walk_kernel (below), which walks it in one lane.
// The counters live in LDS in several copies (a lane takes copy lane % copies, as gs_seen_sweep_kernel): the records of a wave name
// few tax ids, and the atomics of one wave on one LDS word go one after the other.  A workgroup adds its copies up and flushes them
// with global atomics into the copy layout that gs_fold_stats_kernel folds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gs_launch.h"
#include "gs_params.h"
#include "gs_snrec.h"

#define GS_SNR_BLOCK 256
#define GS_SNR_LDS (48 * 1024)                        // bytes of LDS the copies may take
#define GS_SNR_KEEP 4                                 // slots of rows of node codes a lane holds (a power of two)
#define GS_SNR_CELLS (GS_N_SUMS + 1 + GS_N_DCOLS)     // 64-bit cells per value: the row of sums, the max key, the doubles

// copies: a power of two, at most 64 (n_values <= GS_NV_LDS: at least four)
static __host__ __device__ __forceinline__ int gs_snr_copies(int n_values) {
    int copies = 1;
    while (copies < 64 && (size_t)2 * copies * n_values * GS_SNR_CELLS * 8 <= GS_SNR_LDS) copies *= 2;
    return copies;
}

// a workgroup's counter copies (laid out per copy as [nv][GS_N_SUMS] sums | [nv] max keys | [nv][GS_N_DCOLS] doubles) into the run's:
// the copies of a cell added up in one order, then one global atomic per touched cell (behind a __syncthreads of the caller's)
static __device__ __forceinline__ void gs_snr_flush(const GsSnReduceParams &P, const u64 *s_all, int copies, int stride) {
    const int nv = P.n_values;
    const size_t ecopy = P.stat_copies > 1 ? (size_t)(blockIdx.x % (unsigned)P.stat_copies) : 0;
    u64 *const g_sums = (u64 *)P.sums + ecopy * (size_t)nv * GS_N_SUMS;
    u64 *const g_max = (u64 *)P.max_keys + ecopy * (size_t)nv;
    double *const g_d = P.dsums + ecopy * (size_t)nv * GS_N_DCOLS;
    const int n_s = nv * GS_N_SUMS;
    for (int i = threadIdx.x; i < stride; i += GS_SNR_BLOCK) {
        if (i < n_s) {
            u64 a = 0;
            for (int c = 0; c < copies; c++) a += s_all[(size_t)c * stride + i];
            if (a) atomicAdd(&g_sums[i], a);
        } else if (i < n_s + nv) {
            u64 a = 0;
            for (int c = 0; c < copies; c++) a = std::max(a, s_all[(size_t)c * stride + i]);
            if (a) atomicMax(&g_max[i - n_s], a);
        } else {
            double a = 0.0;
            for (int c = 0; c < copies; c++) a += reinterpret_cast<const double *>(s_all)[(size_t)c * stride + i];
            if (a != 0.0) atomicAdd(&g_d[i - n_s - nv], a);
        }
    }
}

// mine (0 .. GS_SNR_KEEP) of every active lane: the sum over the lanes below this one, and over all of them
static __device__ __forceinline__ void gs_snr_wave_prefix(int mine, int lane, unsigned int &before, unsigned int &total) {
    const u64 lt = (1ULL << lane) - 1ULL;
    before = total = 0;
#pragma unroll
    for (int bit = 0; bit < 3; bit++) {  // (GS_SNR_KEEP <= 4)
        const u64 bm = __ballot((mine >> bit) & 1);
        before += (unsigned int)__popcll(bm & lt) << bit;
        total += (unsigned int)__popcll(bm) << bit;
    }
}

__global__ __launch_bounds__(GS_SNR_BLOCK) void gs_sn_reduce_kernel(GsSnReduceParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_snr_lds[];
    __shared__ unsigned int s_booked, s_list_base, s_wave_rows[GS_SNR_BLOCK / 64];
    const int nv = P.n_values;
    const int copies = gs_snr_copies(nv);
    const int stride = nv * GS_SNR_CELLS;  // cells per copy: [nv][GS_N_SUMS] sums | [nv] max keys | [nv][GS_N_DCOLS] doubles
    u64 *const s_all = reinterpret_cast<u64 *>(gs_snr_lds);
    for (int i = threadIdx.x; i < copies * stride; i += GS_SNR_BLOCK) s_all[i] = 0;  // (0.0 is all bits zero)
    if (threadIdx.x == 0) s_booked = 0;
    __syncthreads();
    u64 *const s_sums = s_all + (size_t)(threadIdx.x & (copies - 1)) * stride;
    u64 *const s_max = s_sums + nv * GS_N_SUMS;
    double *const s_d = reinterpret_cast<double *>(s_max + nv);
    const int64_t n = P.count != nullptr ? (int64_t)*P.count : P.n_reads;
    unsigned int mine = 0;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    uint32_t keep[GS_SNR_KEEP];
    int kept = 0;
#pragma unroll
    for (int k = 0; k < GS_SNR_KEEP; k++) keep[k] = 0;
    for (int64_t i = (int64_t)blockIdx.x * GS_SNR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_SNR_BLOCK) {
        // (vi and r first: only a read of one tax id wrote the masks)
        const uint2 head = *reinterpret_cast<const uint2 *>(&P.recs[i].vi);
        const int vi = (int)head.x;
        const uint32_t r = head.y;
        const bool mine_r = (int64_t)r < P.n_reads;
        // A row of node codes is not walked here: 120 steps in one lane would stall the other 63.  A lane keeps the slots of the rows
        // it meets in registers (one record in forty is a row, a lane meets about twenty), and the workgroup places them in the
        // device's list at its end with one atomic; gs_sn_walk_kernel takes the list one lane per read.  A wave in which a lane
        // has GS_SNR_KEEP of them (a batch of little else) places what its lanes hold right away, with one atomic of its own.
        if (vi == GS_SN_NODES && mine_r) {
#pragma unroll
            for (int k = 0; k < GS_SNR_KEEP; k++)
                if (kept == k) keep[k] = (uint32_t)i;
            kept++;
        }
        if (__ballot(kept == GS_SNR_KEEP) != 0) {
            const u64 act = __ballot(true);  // (the lanes still in the loop; the others keep theirs for the end)
            unsigned int before, total;
            gs_snr_wave_prefix(kept, lane, before, total);
            const int leader = __builtin_ctzll(act);
            unsigned int base = 0;
            if (lane == leader) base = atomicAdd(P.n_rows, total);
            base = (unsigned int)__shfl((int)base, leader) + before;
#pragma unroll
            for (int k = 0; k < GS_SNR_KEEP; k++)
                if (k < kept) P.row_list[base + k] = keep[k];
            kept = 0;
        }
        if (vi == GS_SN_NONE && mine_r) {  // no hit, no non-CGAT byte: nothing is booked
            if (P.class_vi) P.class_vi[r] = -1;
            if (P.flags) P.flags[r] = 0;
        }
        if (vi >= 0 && vi < nv && mine_r) {
            const ulonglong2 hits = *reinterpret_cast<const ulonglong2 *>(&P.recs[i].hit0);
            if ((hits.x | hits.y) != 0 && !(P.c.max < 128 && (hits.y >> (P.c.max - 64)) != 0)) {  // (else: no record of the match kernel's)
                GsSnRow row;
                gs_sn_row(hits.x, hits.y, vi, P.c, P.quot, row);
                mine++;
                if (P.class_vi) P.class_vi[r] = row.out_class;
                if (P.flags) P.flags[r] = (uint8_t)row.out_flags;
                u64 *const cell = s_sums + (size_t)vi * GS_N_SUMS;
#pragma unroll
                for (int c = 0; c < GS_N_SUMS; c++)
                    if (row.sums[c]) atomicAdd(&cell[c], (u64)row.sums[c]);
                atomicMax(&s_max[vi], gs_sn_max_key(row.longest, P.first_read_no, r));
                if (row.counted) {
                    double *const d = s_d + (size_t)vi * GS_N_DCOLS;
                    const GsQuotEntry te = P.quot->e[row.tax_err], ce = P.quot->e[row.class_err];
                    atomicAdd(&d[GS_D_ERR_SUM], te.q);
                    atomicAdd(&d[GS_D_ERR_SQ_SUM], te.q2);
                    atomicAdd(&d[GS_D_CLASS_ERR_SUM], ce.q);
                    atomicAdd(&d[GS_D_CLASS_ERR_SQ_SUM], ce.q2);
                }
            }
        }
    }
    if (mine) atomicAdd(&s_booked, mine);
    __syncthreads();
    gs_snr_flush(P, s_all, copies, stride);
    if (threadIdx.x == 0 && s_booked != 0) atomicAdd(P.booked, s_booked);
    // the rows the lanes hold into the device's list (every listed slot is below the record count, and the list has room for n_reads)
    unsigned int before, total;
    gs_snr_wave_prefix(kept, lane, before, total);
    if (lane == 0) s_wave_rows[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int sum = 0;
        for (int i = 0; i < GS_SNR_BLOCK / 64; i++) sum += s_wave_rows[i];
        s_list_base = sum ? atomicAdd(P.n_rows, sum) : 0u;
    }
    __syncthreads();
    unsigned int place = s_list_base + before;
    for (int i = 0; i < wave; i++) place += s_wave_rows[i];
#pragma unroll
    for (int k = 0; k < GS_SNR_KEEP; k++)
        if (k < kept) P.row_list[place + k] = keep[k];
}

// ---------------------------------------------------------------------------------------------------
// gs_sn_walk_kernel: the reads that left the match kernel as rows of node codes, ONE LANE PER READ (gs_sn_walk, gs_snrec.h).  About
// 1.5 % of a batch of genome reads; the per-lane lists of distinct nodes and paths live in scratch.  Counters as above, but in one
// LDS copy per wave: a read books a handful of contigs, and the lanes of a wave are at different positions of different reads.
// ---------------------------------------------------------------------------------------------------
struct GsSnLdsSink {
    u64 *sums, *maxk;
    double *d;
    __device__ __forceinline__ void add(int vi, int col, u64 v) { atomicAdd(&sums[(size_t)vi * GS_N_SUMS + col], v); }
    __device__ __forceinline__ void max_key(int vi, u64 key) { atomicMax(&maxk[vi], key); }
    __device__ __forceinline__ void dadd(int vi, int col, double v) { atomicAdd(&d[(size_t)vi * GS_N_DCOLS + col], v); }
};

// (four waves per SIMD, 128 VGPRs: with more registers on offer the compiler keeps the three lists in registers, indexes them with
// chains of selects and spills 226 scalars)
__global__ __launch_bounds__(GS_SNR_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void gs_sn_walk_kernel(GsSnReduceParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_snr_lds[];
    const int64_t n = (int64_t)*P.n_rows;
    if ((int64_t)blockIdx.x * GS_SNR_BLOCK >= n) return;  // (the grid is sized for a batch of nothing but such reads)
    const int nv = P.n_values;
    const int copies = std::min(gs_snr_copies(nv), GS_SNR_BLOCK / 64);
    const int stride = nv * GS_SNR_CELLS;  // cells per copy, laid out as in gs_sn_reduce_kernel
    u64 *const s_all = reinterpret_cast<u64 *>(gs_snr_lds);
    int32_t *const s_tree = reinterpret_cast<int32_t *>(s_all + (size_t)copies * stride);
    for (int i = threadIdx.x; i < copies * stride; i += GS_SNR_BLOCK) s_all[i] = 0;
    for (int i = threadIdx.x; i < nv; i += GS_SNR_BLOCK) {
        s_tree[i] = P.parent[i];
        s_tree[nv + i] = P.tin[i];
        s_tree[2 * nv + i] = P.tout[i];
    }
    __syncthreads();
    GsSnLdsSink sink;
    sink.sums = s_all + (size_t)((threadIdx.x >> 6) & (copies - 1)) * stride;
    sink.maxk = sink.sums + nv * GS_N_SUMS;
    sink.d = reinterpret_cast<double *>(sink.maxk + nv);
    GsSnWalkConst w;
    w.c = P.c;
    w.max_paths = P.max_paths;
    w.n_values = nv;
    w.parent = s_tree;
    w.tin = s_tree + nv;
    w.tout = s_tree + 2 * nv;
    const int64_t n_recs = P.count != nullptr ? (int64_t)*P.count : P.n_reads;
    for (int64_t i = (int64_t)blockIdx.x * GS_SNR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_SNR_BLOCK) {
        const int64_t slot = (int64_t)P.row_list[i];
        if (slot >= n_recs) continue;  // (no slot of this launch)
        const uint2 head = *reinterpret_cast<const uint2 *>(&P.recs[slot].vi);
        const uint32_t r = head.y;
        if ((int)head.x != GS_SN_NODES || (int64_t)r >= P.n_reads) continue;
        int32_t out_class, out_flags;
        gs_sn_walk(P.nodes + (size_t)slot * GS_SN_ROW, P.recs[slot].bad, r, P.first_read_no, w, P.quot, sink, out_class, out_flags);
        if (P.class_vi) P.class_vi[r] = out_class;
        if (P.flags) P.flags[r] = (uint8_t)out_flags;
    }
    __syncthreads();
    gs_snr_flush(P, s_all, copies, stride);
}

// n_reads: upper bound of the record count (the kernels read the real one from *P->count when there is a survivor list).  The walk
// kernel's grid is sized for a batch of nothing but rows; its workgroups beyond *P->n_rows return at once.
extern "C" hipError_t gs_launch_sn_reduce(const GsSnReduceParams *P, hipStream_t stream) {
    if (P->n_reads <= 0) return hipSuccess;
    if (P->n_values < 1 || P->n_values > GS_NV_LDS || P->row_list == nullptr || P->n_rows == nullptr || P->nodes == nullptr)
        return hipErrorInvalidValue;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((P->n_reads + 4 * GS_SNR_BLOCK - 1) / (4 * GS_SNR_BLOCK), 1024));
    const size_t lds = (size_t)gs_snr_copies(P->n_values) * P->n_values * GS_SNR_CELLS * 8;
    hipLaunchKernelGGL(gs_sn_reduce_kernel, dim3(grid), dim3(GS_SNR_BLOCK), lds, stream, *P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int wgrid = (int)std::max<int64_t>(1, std::min<int64_t>((P->n_reads + GS_SNR_BLOCK - 1) / GS_SNR_BLOCK, 1024));
    const size_t wlds = (size_t)std::min(gs_snr_copies(P->n_values), GS_SNR_BLOCK / 64) * P->n_values * GS_SNR_CELLS * 8 +
                        (size_t)P->n_values * 3 * sizeof(int32_t);
    hipLaunchKernelGGL(gs_sn_walk_kernel, dim3(wgrid), dim3(GS_SNR_BLOCK), wlds, stream, *P);
    return hipGetLastError();
}
