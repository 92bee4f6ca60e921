// stand-in for <hip/hip_runtime.h> on the host (tests/native/accmap_emulate.cpp): the HIP constructs gs_accmap.hip uses; a block is
// 256 real threads, a wave 64 of them; ballot / shuffle are exchanges through memory; streams are the calling thread
#pragma once
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <barrier>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
typedef int hipError_t;
typedef void *hipStream_t;
#define hipSuccess 0
enum { hipMemcpyDeviceToHost = 2 };
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
extern thread_local dim3 threadIdx, blockIdx;
extern std::barrier<> *g_block_bar;
extern std::barrier<> *g_wave_bar[4];
extern unsigned long long g_xch[4][64];
inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
// lane l of the wave reads what lane src(l) wrote
template <class F>
inline unsigned long long emu_exchange(unsigned long long v, F src) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = v;
    g_wave_bar[w]->arrive_and_wait();
    const int s = src(l);
    const unsigned long long r = s >= 0 && s < 64 ? g_xch[w][s] : v;
    g_wave_bar[w]->arrive_and_wait();
    return r;
}
inline unsigned long long __ballot(int pred) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = pred ? 1 : 0;
    g_wave_bar[w]->arrive_and_wait();
    unsigned long long m = 0;
    for (int i = 0; i < 64; i++) m |= g_xch[w][i] << i;
    g_wave_bar[w]->arrive_and_wait();
    return m;
}
inline unsigned long long __shfl_up(unsigned long long v, int d) { return emu_exchange(v, [d](int l) { return l - d; }); }
inline int __shfl(int v, int src) { return (int)(uint32_t)emu_exchange((uint32_t)v, [src](int) { return src; }); }
inline int __ffsll(unsigned long long x) { return __builtin_ffsll((long long)x); }
inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
inline int __popc(uint32_t x) { return __builtin_popcount(x); }
inline int __clz(uint32_t x) { return x ? __builtin_clz(x) : 32; }
template <class T>
inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline uint32_t atomicMax(uint32_t *p, uint32_t v) {
    uint32_t old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}
inline uint32_t atomicMin(uint32_t *p, uint32_t v) {
    uint32_t old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return old;
}
template <class K, class... A>
void emu_launch(K k, dim3 grid, dim3 block, A... a) {
    for (unsigned b = 0; b < grid.x; b++) {
        std::barrier<> bb(block.x), w0(64), w1(64), w2(64), w3(64);
        g_block_bar = &bb; g_wave_bar[0] = &w0; g_wave_bar[1] = &w1; g_wave_bar[2] = &w2; g_wave_bar[3] = &w3;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block.x; t++) th.emplace_back([=] { threadIdx = dim3(t); blockIdx = dim3(b); k(a...); });
        for (auto &x : th) x.join();
    }
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch(k, g, b, __VA_ARGS__)

// stand-in for the one rocPRIM call of the finish: a stable sort of (key, value) pairs between two buffers
#include <algorithm>
#include <numeric>
namespace rocprim {
template <class T>
struct double_buffer {
    T *bufs[2];
    int sel = 0;
    double_buffer(T *a, T *b) : bufs{a, b} {}
    T *current() const { return bufs[sel]; }
    T *alternate() const { return bufs[sel ^ 1]; }
    void swap() { sel ^= 1; }
};
template <class K, class V>
hipError_t radix_sort_pairs(void *tmp, size_t &tmp_bytes, double_buffer<K> &keys, double_buffer<V> &vals, size_t n, unsigned, unsigned, hipStream_t) {
    if (!tmp) {
        tmp_bytes = 16;
        return 0;
    }
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return keys.current()[a] < keys.current()[b]; });
    for (size_t i = 0; i < n; i++) {
        keys.alternate()[i] = keys.current()[order[i]];
        vals.alternate()[i] = vals.current()[order[i]];
    }
    keys.swap();
    vals.swap();
    return 0;
}
}  // namespace rocprim
