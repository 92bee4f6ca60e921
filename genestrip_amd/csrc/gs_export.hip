// gs_export.hip -- the device store read back (include/gsgpu.h, gs_db_value_counts / gs_dbexport_*): the counterpart of the
// reference's KMerStore.visit (C/store/KMerSortedArray.java:426-439), Database.getStats (C/store/Database.java:159) and
// KMerFastqGenerator + FastQWriter (C/fastqgen/).
//   every record line and table bucket of a handle's store -> (reference key, value index) of each stored k-mer   gs_ex_decode_kernel
//   the pairs sorted by key (ascending: KMerSortedArray.visit order)                                            gs_build_sort (gs_build.hip)
//   per selected k-mer one FASTQ record: lengths, exclusive scan, bytes                                          gs_ex_fastq_*_kernel
// The layout is reversible: a record line holds its whole window (planes + valid bits + value indices), a table slot holds
// rem | disp | value + 1, and gs_mix_planes is a Feistel bijection (gs_unmix_planes).  Seen bits (a live unique-counting run)
// and `more` bits are masked, so an export may run beside a match.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "gs_decode.h"  // the walk's loads and field decoders, shared with gs_index.hip
#include "gs_launch.h"
#include "gs_layout.h"

#define GS_EX_BLOCK 256
#define GS_EX_LDS_BINS 16384  // value counts privatised in LDS up to this many values (64 KiB)

__device__ __forceinline__ bool gs_ex_selected(const GsExportParams &P, int32_t v) {
    if (P.sel_vi < 0) return true;
    if (!P.with_desc) return v == P.sel_vi;
    const int32_t t = P.tin[v];
    return P.tin[P.sel_vi] <= t && t < P.tout[P.sel_vi];
}

// The walk of gs_decode.h: four lanes per 64-byte line.  Each lane emits at most GS_EX_MAX_PER_LANE k-mers; the wave places them
// through a ballot prefix over the three bits of the per-lane count and one atomic add.
__global__ __launch_bounds__(GS_EX_BLOCK) void gs_ex_decode_kernel(GsExportParams P) {
    extern __shared__ unsigned int lds_hist[];
    const bool lds = P.hist && P.n_values <= GS_EX_LDS_BINS;
    if (lds) {
        for (int i = threadIdx.x; i < P.n_values; i += blockDim.x) lds_hist[i] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, q = lane & 3;
    const int64_t n_lines = P.n_rec + P.n_tab;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint32_t kmask = (uint32_t)((1ULL << P.k) - 1);
    const uint32_t vmask = (1u << P.vbits) - 1u;
    // (the loop bound is uniform per wave: lines are whole quads, a quad never straddles a wave)
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); t0 < 4 * n_lines; t0 += stride) {
        const int64_t t = t0 + lane;
        const int64_t line = t >> 2;
        u64 x0, x1;
        const bool is_rec = line < P.n_rec;
        gs_ex_load_quad(P.rec, P.tab, P.n_rec, n_lines, line, q, x0, x1);
        const int src = lane & ~3;
        const u64 w0 = __shfl(x0, src), w1 = __shfl(x1, src);
        // which of the lane's (up to six) entries it emits: bit i = record offset 6 (q - 1) + i / table slot 2 q + i
        uint32_t sel = 0;
        if (line < n_lines) {
            if (is_rec) {
                const uint32_t valid = gs_ex_rec_valid(w1, q);
                for (int i = 0; i < GS_EX_MAX_PER_LANE; i++)
                    if ((valid >> i) & 1u) {
                        const int32_t v = gs_ex_rec_value(x0, x1, i);
                        if (v < P.n_values && gs_ex_selected(P, v)) sel |= 1u << i;
                    }
            } else {
                for (int i = 0; i < 2; i++) {
                    const int32_t v = gs_ex_tab_value(i ? x1 : x0, vmask);
                    if (v >= 0 && v < P.n_values && gs_ex_selected(P, v)) sel |= 1u << i;
                }
            }
        }
        // wave prefix of the per-lane counts (0..6) from three ballots, one atomic per wave
        int before, total;
        gs_ex_wave_prefix(__popc(sel), lane, before, total);
        if (total == 0) continue;
        u64 base = 0;
        if (lane == 0) base = atomicAdd(P.count, (u64)total);
        base = __shfl(base, 0) + (u64)before;
        for (uint32_t m = sel; m; m &= m - 1, base++) {
            const int i = __builtin_ctz(m);
            uint32_t v;
            u64 key = 0;
            if (is_rec) {
                v = (uint32_t)gs_ex_rec_value(x0, x1, i);
                if (P.keys) key = gs_ex_rec_key(w0, w1, 6 * (q - 1) + i, P.k, kmask);
            } else {
                const u64 s = i ? x1 : x0;
                v = (uint32_t)gs_ex_tab_value(s, vmask);
                if (P.keys) key = gs_ex_tab_key(s, (u64)(P.tab_first + (line - P.n_rec)), P.vbits, P.bucket_bits, P.k, kmask);
            }
            if (P.keys && base < P.cap) {
                P.keys[base] = key;
                P.vals[base] = v;
            }
            if (P.hist) {
                if (lds)
                    atomicAdd(&lds_hist[v], 1u);
                else
                    atomicAdd(&P.hist[v], 1ULL);
            }
        }
    }
    if (lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < P.n_values; i += blockDim.x)
            if (lds_hist[i]) atomicAdd(&P.hist[i], (u64)lds_hist[i]);
    }
}

extern "C" hipError_t gs_launch_export_decode(const GsExportParams *P, int n_cu, hipStream_t stream) {
    const int64_t threads = 4 * (P->n_rec + P->n_tab);
    if (threads == 0) return hipSuccess;
    int64_t grid = (threads + GS_EX_BLOCK - 1) / GS_EX_BLOCK;
    const int64_t cap = (int64_t)n_cu * 8;  // grid-stride beyond ~8 workgroups per CU (the LDS histogram is flushed once per workgroup)
    if (grid > cap) grid = cap;
    const size_t lds = P->hist && P->n_values <= GS_EX_LDS_BINS ? (size_t)P->n_values * sizeof(unsigned int) : 0;
    hipLaunchKernelGGL(gs_ex_decode_kernel, dim3((unsigned)grid), dim3(GS_EX_BLOCK), lds, stream, *P);
    return hipGetLastError();
}

// ---- FASTQ text (FastQWriter.addRead as called by KMerFastqGenerator.generateFastq):
//   "@GENESTRIP:" project ":" ":" taxid ":" n "\n" bases "\n" "+\n" '~' x k "\n"       n = 1, 2, .. over the file

__device__ __forceinline__ int gs_ex_digits(u64 x) {
    int d = 1;
    while (x >= 10) {
        x /= 10;
        d++;
    }
    return d;
}

__global__ __launch_bounds__(GS_EX_BLOCK) void gs_ex_fastq_len_kernel(GsFastqParams P) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < P.n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t v = P.vals[P.first + r];
        const uint32_t tl = P.name_off[v + 1] - P.name_off[v];
        P.len[r] = 19u + (uint32_t)P.project_len + tl + (uint32_t)gs_ex_digits((u64)(P.first + r + 1)) + 2u * (uint32_t)P.k;
    }
}

__global__ __launch_bounds__(GS_EX_BLOCK) void gs_ex_fastq_write_kernel(GsFastqParams P) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < P.n; r += (int64_t)gridDim.x * blockDim.x) {
        uint8_t *o = P.text + P.off[r];
        const uint32_t v = P.vals[P.first + r];
        const char *id = "@GENESTRIP:";
        for (int i = 0; i < 11; i++) *o++ = (uint8_t)id[i];
        for (int i = 0; i < P.project_len; i++) *o++ = P.project[i];
        *o++ = ':';
        *o++ = ':';
        for (uint32_t i = P.name_off[v]; i < P.name_off[v + 1]; i++) *o++ = P.names[i];
        *o++ = ':';
        u64 num = (u64)(P.first + r + 1);
        const int d = gs_ex_digits(num);
        for (int i = d - 1; i >= 0; i--) {
            o[i] = (uint8_t)('0' + num % 10);
            num /= 10;
        }
        o += d;
        *o++ = '\n';
        const u64 key = P.keys[P.first + r];  // CGAT.longToKMerStraight: first base in the top bits, C G A T = 0 1 2 3
        for (int i = 0; i < P.k; i++) *o++ = (uint8_t)"CGAT"[(key >> (2 * (P.k - 1 - i))) & 3u];
        *o++ = '\n';
        *o++ = '+';
        *o++ = '\n';
        for (int i = 0; i < P.k; i++) *o++ = '~';
        *o++ = '\n';
    }
}

static unsigned gs_ex_grid(int64_t n) {
    const int64_t g = (n + GS_EX_BLOCK - 1) / GS_EX_BLOCK;
    return (unsigned)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

// P->len / P->off: n + 1 entries; scratch / scratch_bytes: rocPRIM temporary storage (call with scratch == nullptr to learn the size)
// text == nullptr: lengths + scan, *n_bytes = text of the n records; then with P->text (room for *n_bytes): the bytes
extern "C" hipError_t gs_launch_export_fastq(const GsFastqParams *P, void *scratch, size_t *scratch_bytes, int64_t *n_bytes, hipStream_t stream) {
    if (!scratch) return rocprim::exclusive_scan(nullptr, *scratch_bytes, P->len, P->off, 0u, (size_t)P->n + 1, rocprim::plus<uint32_t>(), stream);
    if (P->n <= 0) {
        *n_bytes = 0;
        return hipSuccess;
    }
    if (!P->text) {
        hipLaunchKernelGGL(gs_ex_fastq_len_kernel, dim3(gs_ex_grid(P->n)), dim3(GS_EX_BLOCK), 0, stream, *P);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemsetAsync(P->len + P->n, 0, sizeof(uint32_t), stream);
        if (e == hipSuccess)
            e = rocprim::exclusive_scan(scratch, *scratch_bytes, P->len, P->off, 0u, (size_t)P->n + 1, rocprim::plus<uint32_t>(), stream);
        uint32_t total = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&total, P->off + P->n, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        *n_bytes = total;
        return e;
    }
    hipLaunchKernelGGL(gs_ex_fastq_write_kernel, dim3(gs_ex_grid(P->n)), dim3(GS_EX_BLOCK), 0, stream, *P);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e;
}
