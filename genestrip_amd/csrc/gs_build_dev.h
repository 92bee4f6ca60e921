// gs_build_dev.h -- device code shared by the one-shot builder (gs_build.hip) and the streaming update (gs_update.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
