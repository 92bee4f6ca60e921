// stand-in for <hip/hip_runtime.h> on the host (tests/native/records_emulate.cpp): what kraken_emulate_hip.h knows, and the
// atomics on 32-bit words that gs_rewrite.hip uses besides
#pragma once
#include "kraken_emulate_hip.h"
inline uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline uint32_t atomicMin(uint32_t *p, uint32_t v) {
    uint32_t old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {
    }
    return old;
}

// The launcher of kraken_emulate_hip.h starts a block's threads anew for every block; the rewrite kernels are many small launches
// (one of them 1024 threads wide), so here the threads live for the whole program and wait for their next block at a barrier.
struct EmuPool {
    static constexpr unsigned kThreads = 1024;
    std::barrier<> start{kThreads + 1}, done{kThreads + 1};
    std::function<void(unsigned)> job;
    unsigned active = 0;
    bool quit = false;
    std::vector<std::thread> th;
    EmuPool() {
        for (unsigned t = 0; t < kThreads; t++)
            th.emplace_back([this, t] {
                for (;;) {
                    start.arrive_and_wait();
                    if (quit) return;
                    if (t < active) job(t);
                    done.arrive_and_wait();
                }
            });
    }
    ~EmuPool() {
        quit = true;
        start.arrive_and_wait();
        for (auto &x : th) x.join();
    }
};
inline EmuPool &emu_pool() {
    static EmuPool p;
    return p;
}
template <class K, class... A>
void emu_pool_launch(K k, dim3 grid, dim3 block, A... a) {
    EmuPool &p = emu_pool();
    gridDim = grid;
    for (unsigned b = 0; b < grid.x; b++) {
        std::barrier<> bb(block.x), w0(64), w1(64), w2(64), w3(64);
        g_block_bar = &bb; g_wave_bar[0] = &w0; g_wave_bar[1] = &w1; g_wave_bar[2] = &w2; g_wave_bar[3] = &w3;
        p.active = block.x;
        p.job = [=](unsigned t) { threadIdx = dim3(t); blockIdx = dim3(b); k(a...); };
        p.start.arrive_and_wait();
        p.done.arrive_and_wait();
    }
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_pool_launch(k, g, b, __VA_ARGS__)
