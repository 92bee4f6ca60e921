// gs_snreduce.hip -- gs_sn_reduce_kernel: the records that the FIXED loop of gs_match_kernel wrote for its reads of one tax id
// (GsSnRec, gs_snrec.h) into the run's counters and per-read outputs.  ONE LANE PER RECORD: contigs, classification, flags and the
// read's row are gs_sn_row, which the match kernel used to work off one read at a time on the scalar unit.
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
#define GS_SNR_CELLS (GS_N_SUMS + 1 + GS_N_DCOLS)     // 64-bit cells per value: the row of sums, the max key, the doubles

// copies: a power of two, at most 64 (n_values <= GS_NV_LDS: at least four)
static __host__ __device__ __forceinline__ int gs_snr_copies(int n_values) {
    int copies = 1;
    while (copies < 64 && (size_t)2 * copies * n_values * GS_SNR_CELLS * 8 <= GS_SNR_LDS) copies *= 2;
    return copies;
}

__global__ __launch_bounds__(GS_SNR_BLOCK) void gs_sn_reduce_kernel(GsSnReduceParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_snr_lds[];
    __shared__ unsigned int s_booked;
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
    for (int64_t i = (int64_t)blockIdx.x * GS_SNR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * GS_SNR_BLOCK) {
        // (vi and r first: a read that was not deferred wrote nothing else, and its slot's masks are of no interest)
        const uint2 head = *reinterpret_cast<const uint2 *>(&P.recs[i].vi);
        const int vi = (int)head.x;
        const uint32_t r = head.y;
        if (vi < 0 || vi >= nv || (int64_t)r >= P.n_reads) continue;
        const ulonglong2 hits = *reinterpret_cast<const ulonglong2 *>(&P.recs[i].hit0);
        if ((hits.x | hits.y) == 0 || (P.c.max < 128 && (hits.y >> (P.c.max - 64)) != 0)) continue;  // (no record of the match kernel's)
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
    if (mine) atomicAdd(&s_booked, mine);
    __syncthreads();
    // the copies of a cell added up in one order, then one global atomic per touched cell
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
    if (threadIdx.x == 0 && s_booked != 0) atomicAdd(P.booked, s_booked);
}

// n_reads: upper bound of the record count (the kernel reads the real one from *P->count when there is a survivor list)
extern "C" hipError_t gs_launch_sn_reduce(const GsSnReduceParams *P, hipStream_t stream) {
    if (P->n_reads <= 0) return hipSuccess;
    if (P->n_values < 1 || P->n_values > GS_NV_LDS) return hipErrorInvalidValue;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((P->n_reads + 4 * GS_SNR_BLOCK - 1) / (4 * GS_SNR_BLOCK), 1024));
    const size_t lds = (size_t)gs_snr_copies(P->n_values) * P->n_values * GS_SNR_CELLS * 8;
    hipLaunchKernelGGL(gs_sn_reduce_kernel, dim3(grid), dim3(GS_SNR_BLOCK), lds, stream, *P);
    return hipGetLastError();
}
