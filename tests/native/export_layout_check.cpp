// Host checks of the store export's layout helpers (genestrip_amd/csrc/gs_layout.h), built with g++:
//   mix      gs_unmix_planes undoes gs_mix_planes on 10^6 random plane pairs and on the edge values (and the other way round)
//   keys     stdin lines "k hi lo" -> stdout "key" = gs_planes_to_kmer(hi, lo, k), for the test's Python restatement
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../genestrip_amd/csrc/gs_layout.h"

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static int check_pair(uint32_t a, uint32_t b) {
    uint32_t x, y;
    const uint64_t h = gs_mix_planes(a, b);
    gs_unmix_planes(h, x, y);
    if (h >> 62 || x != a || y != b) {
        printf("mismatch a=%08x b=%08x h=%016" PRIx64 " -> %08x %08x\n", a, b, h, x, y);
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "mix")) {
        int fails = 0;
        const uint32_t edge[] = {0u, 1u, 2u, 0x7ffffffeu, 0x7fffffffu, 0x40000000u, 0x3fffffffu, 0x55555555u, 0x2aaaaaaau};
        for (uint32_t a : edge)
            for (uint32_t b : edge) fails += check_pair(a, b);
        uint64_t s = 12345;
        for (int i = 0; i < 1000000; i++) {
            const uint64_t r = splitmix(s);
            fails += check_pair((uint32_t)r & 0x7fffffffu, (uint32_t)(r >> 32) & 0x7fffffffu);
            const uint64_t h = splitmix(s) >> 2;  // any h < 2^62 is the image of exactly one pair
            uint32_t x, y;
            gs_unmix_planes(h, x, y);
            if (x >> 31 || y >> 31 || gs_mix_planes(x, y) != h) fails++;
        }
        printf("fails %d\n", fails);
        return fails != 0;
    }
    if (argc > 1 && !strcmp(argv[1], "keys")) {
        int k;
        uint32_t hi, lo;
        while (scanf("%d %u %u", &k, &hi, &lo) == 3) printf("%" PRIu64 "\n", gs_planes_to_kmer(hi, lo, k));
        return 0;
    }
    fprintf(stderr, "usage: %s mix | keys\n", argv[0]);
    return 2;
}
