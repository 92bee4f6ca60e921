// The byte -> 15-mer conversion and the two-level probe of genestrip_amd/csrc/gs_prefilter.h compiled for the host, held to the
// Python restatement (tests/prefilter.py) on a case file that tests/test_prefilter_cpu.py writes:
//   int32 k, L, n_reads, n_samples; int64 n_set; int64 set[n_set] (canonical codes of S); uint8 reads[n_reads * L];
//   int64 canon[n_reads * n_samples]; uint8 bad[n_reads * n_samples]; uint8 pass[n_reads]
// Every buffer is exactly as large as its contents: a read of a byte beyond a read's samples is AddressSanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../genestrip_amd/csrc/gs_prefilter.h"

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    int64_t n_set = 0;
    if (!get(f, head, 4) || !get(f, &n_set, 1)) return 2;
    const int k = head[0], L = head[1], n = head[2], m = head[3];
    std::vector<int64_t> set((size_t)n_set), canon((size_t)n * m);
    std::vector<uint8_t> bad((size_t)n * m), pass((size_t)n);
    std::vector<std::vector<uint8_t>> reads((size_t)n, std::vector<uint8_t>((size_t)L));  // one allocation per read
    bool ok = get(f, set.data(), set.size());
    for (int r = 0; ok && r < n; r++) ok = get(f, reads[r].data(), (size_t)L);
    ok = ok && get(f, canon.data(), canon.size()) && get(f, bad.data(), bad.size()) && get(f, pass.data(), pass.size());
    fclose(f);
    if (!ok) return 2;
    int fails = 0;
    if (gs_pf_samples(L, k) != m) {
        printf("MISMATCH samples %d, the restatement has %d\n", gs_pf_samples(L, k), m);
        fails++;
    }
    std::vector<uint32_t> l1((size_t)1 << (GS_PF_L1_BITS - 5), 0u), l2(GS_PF_L2_WORDS, 0u);
    for (int64_t c : set) {
        l2[(size_t)c >> 5] |= 1u << (c & 31);
        const uint32_t b = gs_pf_l1_bit((uint32_t)c);
        l1[b >> 5] |= 1u << (b & 31);
    }
    int n_pass = 0;
    for (int r = 0; r < n && fails < 20; r++) {
        for (int i = 0; i < m; i++) {
            const uint8_t *p = reads[r].data() + i * gs_pf_stride(k);
            uint32_t d[4] = {0, 0, 0, 0};
            for (int j = 0; j < GS_MIN_L; j++) d[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
            const bool is_bad = gs_pf_bad15(d[0], d[1], d[2], d[3]) != 0;
            if (is_bad != (bad[(size_t)r * m + i] != 0)) {
                printf("MISMATCH read %d sample %d: bad %d\n", r, i, (int)is_bad);
                fails++;
            } else if (!is_bad && (int64_t)gs_pf_canon15(d[0], d[1], d[2], d[3]) != canon[(size_t)r * m + i]) {
                printf("MISMATCH read %d sample %d: code %u, the restatement has %lld\n", r, i, gs_pf_canon15(d[0], d[1], d[2], d[3]),
                       (long long)canon[(size_t)r * m + i]);
                fails++;
            }
        }
        const bool got = gs_pf_read_passes(l1.data(), l2.data(), reads[r].data(), L, k);
        n_pass += got;
        if (got != (pass[r] != 0)) {
            printf("MISMATCH read %d: passes %d\n", r, (int)got);
            fails++;
        }
    }
    printf("k %d L %d: %d reads, %d pass, fails %d\n", k, L, n, n_pass, fails);
    if (!fails) printf("case ok\n");
    return fails ? 1 : 0;
}
