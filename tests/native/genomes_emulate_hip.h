// stand-in for <hip/hip_runtime.h> on the host (tests/native/genomes_emulate.cpp): what records_emulate_hip.h knows, and the few
// constructs gs_genomes.hip uses besides
#pragma once
#include <algorithm>
#include "records_emulate_hip.h"
using std::max;
using std::min;
inline int __popc(uint32_t x) { return __builtin_popcount(x); }
inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline uint32_t atomicMax(uint32_t *p, uint32_t v) {
    uint32_t old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {
    }
    return old;
}
