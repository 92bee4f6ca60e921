// gs_build_dev.h -- device code shared by the one-shot builder (gs_build.hip), the streaming update (gs_update.hip) and the
// sizing pass (gs_size.hip): the common ancestor, and the tile decode of the k-mer kernels (code, planes -> k-mer, DUST)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned long long u64;

// TaxTree.getLowestCommonAncestor (C/tax/TaxTree.java:160-187) over value indices; one tree (the API refuses forests)
__device__ __forceinline__ int gs_build_lca(const int32_t *parent, const int32_t *depth, int a, int b) {
    while (depth[a] > depth[b]) a = parent[a];
    while (depth[b] > depth[a]) b = parent[b];
    while (a != b) {
        a = parent[a];
        b = parent[b];
    }
    return a;
}

// 2-bit code of the reference (C/util/CGAT.java:66-74: C0 G1 A2 T3), 4 = not a base.  lower: enableLowerCaseBases
// (AbstractStoreFastaReader.java:100: CGAT.cgatToUpperCase)
__device__ __forceinline__ uint32_t gs_build_code(uint8_t c, int lower) {
    if (lower && c >= 'a') c = (uint8_t)(c - 32);
    return c == 'C' ? 0u : c == 'G' ? 1u : c == 'A' ? 2u : c == 'T' ? 3u : 4u;
}

// bit i of v -> bit 2 i
__device__ __forceinline__ u64 gs_build_spread(uint32_t v) {
    u64 x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFULL;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFULL;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0FULL;
    x = (x | (x << 2)) & 0x3333333333333333ULL;
    x = (x | (x << 1)) & 0x5555555555555555ULL;
    return x;
}

// The reference's low-complexity score of a k-mer (CGATLongBuffer.getDustValue, C/util/CGATLongBuffer.java:146-229; its test
// T/util/CGATLongBufferTest.java:280-313 states it for a window): for the periods 1, 2, 3 every maximal run of L consecutive
// positions whose base equals the base `period` earlier adds fib(L), fib = 0, 1, 2, 3, 5, 8 ...  On planes: one mask of matches
// per period, then a walk over its runs of ones.
__device__ __forceinline__ int gs_build_dust(uint32_t fhi, uint32_t flo, int k) {
    int d = 0;
    for (int p = 1; p <= 3 && p < k; p++) {
        uint32_t m = ~((fhi ^ (fhi >> p)) | (flo ^ (flo >> p))) & ((1u << (k - p)) - 1u);
        while (m) {
            m >>= __builtin_ctz(m);
            const int len = __builtin_ctz(~m);  // (m < 2^31: a zero bit always follows)
            int a = 1, b = 2;                   // fib(1), fib(2)
            for (int i = 1; i < len; i++) {
                const int c = a + b;
                a = b;
                b = c;
            }
            d += a;
            m >>= len;
        }
    }
    return d;
}

// k bits of the 128-bit string {b (high), a (low)} from bit s (s in 0..63, k <= 31)
__device__ __forceinline__ uint32_t gs_build_funnel(u64 a, u64 b, int s, uint32_t kmask) {
    return (uint32_t)((a >> s) | ((b << 1) << (63 - s))) & kmask;
}
