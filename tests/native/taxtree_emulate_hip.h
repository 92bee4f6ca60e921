// stand-in for <hip/hip_runtime.h> and the rocPRIM headers on the host (tests/native/taxtree_emulate.cpp): what accmap_emulate_hip.h
// has, and the further constructs gs_taxtree.hip uses
#pragma once
#include "accmap_emulate_hip.h"
#define __constant__ static const
enum { hipMemcpyDeviceToDevice = 3 };
inline int32_t atomicCAS(int32_t *p, int32_t expect, int32_t v) {
    __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
    return expect;
}
inline unsigned long long atomicMax(unsigned long long *p, unsigned long long v) {
    unsigned long long old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}
inline int __shfl_xor(int v, int mask) { return (int)(uint32_t)emu_exchange((uint32_t)v, [mask](int l) { return l ^ mask; }); }
namespace rocprim {
template <class T>
struct plus {
    T operator()(T a, T b) const { return a + b; }
};
template <class K>
hipError_t radix_sort_keys(void *tmp, size_t &tmp_bytes, double_buffer<K> &keys, size_t n, unsigned, unsigned, hipStream_t) {
    if (!tmp) {
        tmp_bytes = 16;
        return 0;
    }
    std::copy(keys.current(), keys.current() + n, keys.alternate());
    std::stable_sort(keys.alternate(), keys.alternate() + n);
    keys.swap();
    return 0;
}
template <class T, class Op>
hipError_t exclusive_scan(void *tmp, size_t &tmp_bytes, const T *in, T *out, T init, size_t n, Op op, hipStream_t) {
    if (!tmp) {
        tmp_bytes = 16;
        return 0;
    }
    T run = init;
    for (size_t i = 0; i < n; i++) {
        const T x = in[i];
        out[i] = run;
        run = op(run, x);
    }
    return 0;
}
}  // namespace rocprim
