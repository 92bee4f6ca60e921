// gs_scan.h -- the exclusive prefix inside a block of GS_SCAN_BLOCK threads that the text stages share (gs_rewrite.hip, gs_kraken.hip):
// sizes per record, scanned inside blocks; the per-block sums go through gs_launch_scan_blocks (gs_rewrite.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#define GS_SCAN_BLOCK 256

// exclusive prefix of v over the block (GS_SCAN_BLOCK threads, every one of them arrives); *total: the block's sum.  s_wave:
// GS_SCAN_BLOCK / 64 words of LDS, free again once every thread has returned and passed one more barrier
__device__ __forceinline__ unsigned long long gs_block_scan(unsigned long long v, unsigned long long *s_wave, unsigned long long *total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long x = __shfl_up(inc, d);
        if (lane >= d) inc += x;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int w = 0; w < GS_SCAN_BLOCK / 64; w++) {
        if (w < wv) before += s_wave[w];
        all += s_wave[w];
    }
    *total = all;
    return before + inc - v;
}
