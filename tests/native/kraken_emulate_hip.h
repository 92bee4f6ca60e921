// stand-in for <hip/hip_runtime.h> on the host (tests/native/kraken_emulate.cpp): the few HIP constructs gs_kraken.hip uses; a block
// is 256 real threads, a wave 64 of them
#pragma once
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <barrier>
#include <thread>
#include <vector>
#include <functional>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
typedef int hipError_t;
typedef void *hipStream_t;
#define hipSuccess 0
inline hipError_t hipGetLastError() { return 0; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { uint32_t x, y, z, w; };
extern thread_local dim3 threadIdx, blockIdx;
extern dim3 gridDim;
extern std::barrier<> *g_block_bar;
extern std::barrier<> *g_wave_bar[4];
extern unsigned long long g_xch[4][64];
inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
inline unsigned long long __ballot(int pred) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = pred ? 1 : 0;
    g_wave_bar[w]->arrive_and_wait();
    unsigned long long m = 0;
    for (int i = 0; i < 64; i++) m |= g_xch[w][i] << i;
    g_wave_bar[w]->arrive_and_wait();
    return m;
}
inline unsigned long long __shfl_up(unsigned long long v, int d) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = v;
    g_wave_bar[w]->arrive_and_wait();
    unsigned long long r = l >= d ? g_xch[w][l - d] : v;
    g_wave_bar[w]->arrive_and_wait();
    return r;
}
inline unsigned long long __shfl_xor(unsigned long long v, int d) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_xch[w][l] = v;
    g_wave_bar[w]->arrive_and_wait();
    unsigned long long r = g_xch[w][l ^ d];
    g_wave_bar[w]->arrive_and_wait();
    return r;
}
inline int __ffsll(long long x) { return __builtin_ffsll(x); }
inline int __popcll(unsigned long long x) { return __builtin_popcountll(x); }
inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
template <class K, class... A>
void emu_launch(K k, dim3 grid, dim3 block, A... a) {
    gridDim = grid;
    for (unsigned b = 0; b < grid.x; b++) {
        std::barrier<> bb(block.x), w0(64), w1(64), w2(64), w3(64);
        g_block_bar = &bb; g_wave_bar[0] = &w0; g_wave_bar[1] = &w1; g_wave_bar[2] = &w2; g_wave_bar[3] = &w3;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < block.x; t++) th.emplace_back([=] { threadIdx = dim3(t); blockIdx = dim3(b); k(a...); });
        for (auto &x : th) x.join();
    }
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch(k, g, b, __VA_ARGS__)
