// gs_checksum.h -- the checksum of the native files (store file, index file): host code only, shared by gs_api.cpp and the
// stand-alone check of the index file reader (tests/native/indexfile_sanitize.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <thread>
#include <vector>

// two running 64-bit sums over the payload's 32-bit words (Fletcher style): position sensitive, one pass
struct StoreChecksum {
    uint64_t a = 1, b = 0;
    // a and b after the words of [p, p + bytes): slices are summed by all cores with a = b = 0 -- S = sum of the words, T = sum
    // of their prefix sums -- and chained: a' = a + S, b' = b + n * a + T (the same numbers as the word-by-word loop, mod 2^64)
    void add(const void *p, size_t bytes) {
        const uint32_t *w = (const uint32_t *)p;
        const size_t n = bytes / 4;
        int n_thr = n < ((size_t)1 << 22) ? 1 : (int)std::min<unsigned>(32, std::max<unsigned>(1, std::thread::hardware_concurrency()));
        std::vector<uint64_t> S((size_t)n_thr, 0), T((size_t)n_thr, 0);
        auto part = [&](int t) {
            const size_t lo = n * (size_t)t / (size_t)n_thr, hi = n * ((size_t)t + 1) / (size_t)n_thr;
            uint64_t sa = 0, sb = 0;
            for (size_t i = lo; i < hi; i++) {
                sa += w[i];
                sb += sa;
            }
            S[(size_t)t] = sa;
            T[(size_t)t] = sb;
        };
        if (n_thr == 1)
            part(0);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < n_thr; t++) th.emplace_back(part, t);
            for (auto &x : th) x.join();
        }
        for (int t = 0; t < n_thr; t++) {
            const size_t lo = n * (size_t)t / (size_t)n_thr, hi = n * ((size_t)t + 1) / (size_t)n_thr;
            b += (uint64_t)(hi - lo) * a + T[(size_t)t];
            a += S[(size_t)t];
        }
    }
    uint64_t value() const { return a ^ (b << 1) ^ (b >> 63); }
};
