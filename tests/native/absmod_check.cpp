// Host check of the filter's magic-number division (genestrip_amd/csrc/gs_absmod.h, the text gs_filter_kernel compiles), built
// with g++: gs_absmod(v, d, gs_magic_u64(d)) against Math.abs(v % d) in 128-bit arithmetic for the divisors a filter can have
// (1 <= d <= 2^37) and the dividends where a division goes wrong.  Prints "cases N fails F".
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../genestrip_amd/csrc/gs_absmod.h"

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// Java's Math.abs(v % d): % truncates toward zero; |v % d| < d, so the abs never overflows
static uint64_t java_absmod(int64_t v, uint64_t d) {
    const __int128 r = (__int128)v % (__int128)d;
    return (uint64_t)(r < 0 ? -r : r);
}

static long long g_cases = 0, g_fails = 0;

static void check(int64_t v, uint64_t d, uint64_t magic, int shift) {
    g_cases++;
    const uint64_t got = gs_absmod(v, d, magic, shift), want = java_absmod(v, d);
    if (got != want && g_fails++ < 20)
        printf("d=%" PRIu64 " v=%" PRId64 " got %" PRIu64 " want %" PRIu64 "\n", d, v, got, want);
}

static void check_divisor(uint64_t d, uint64_t &rng) {
    uint64_t magic = 0;
    int shift = -1;
    gs_magic_u64(d, magic, shift);
    if ((shift == 0) != (d == 1)) {
        g_fails++;
        printf("d=%" PRIu64 " shift %d\n", d, shift);
    }
    const int64_t MAX = INT64_MAX, MIN = INT64_MIN;
    std::vector<int64_t> vs = {0, 1, 2, MAX, MAX - 1, MIN, MIN + 1, MIN + 2, -1, -2};
    // n = m * d + e and -n, in u64 arithmetic (m * d + 1 may be 2^63, whose negation is INT64_MIN)
    auto both = [&](uint64_t n) {
        vs.push_back((int64_t)n);
        vs.push_back((int64_t)((uint64_t)0 - n));
    };
    const uint64_t top = (uint64_t)MAX / d;  // multiples of d across the whole range
    for (uint64_t e : {(uint64_t)-1, (uint64_t)0, (uint64_t)1}) {
        both(d + e);
        both(d - 1 + e);
        for (uint64_t m : {(uint64_t)2, (uint64_t)3, (uint64_t)1 << 20, top / 2 + 1, top - 1, top})
            if (m >= 1 && m <= top) both(m * d + e);
    }
    for (int i = 0; i < 64; i++) vs.push_back((int64_t)splitmix(rng));
    for (int i = 0; i < 16; i++) vs.push_back((int64_t)(splitmix(rng) >> (i + 20)));
    for (int64_t v : vs) check(v, d, magic, shift);
}

int main() {
    uint64_t rng = 0x5EED;
    std::vector<uint64_t> ds = {1, 2, 3, 5, 7, 63, 64, 65};
    for (int j = 1; j <= 37; j++) {
        ds.push_back(((uint64_t)1 << j) - 1);
        ds.push_back((uint64_t)1 << j);
        ds.push_back(((uint64_t)1 << j) + 1);
    }
    // primes: 2^31 - 1, 2^32 - 5, 2^33 - 9, 2^36 - 5, 2^37 - 25, 10^9 + 7, 999999937
    for (uint64_t p : {2147483647ULL, 4294967291ULL, 8589934583ULL, 68719476731ULL, 137438953447ULL, 1000000007ULL, 999999937ULL})
        ds.push_back(p);
    for (int i = 0; i < 20000; i++) ds.push_back(1 + splitmix(rng) % ((uint64_t)1 << 37));
    for (int i = 0; i < 2000; i++) ds.push_back(1 + splitmix(rng) % 100000);
    for (uint64_t d : ds) check_divisor(d, rng);
    printf("cases %lld fails %lld\n", g_cases, g_fails);
    return g_fails != 0;
}
