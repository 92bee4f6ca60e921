// The per-record arithmetic of gs_sn_reduce_kernel (gs_sn_row, genestrip_amd/csrc/gs_snrec.h), compiled for the host under
// AddressSanitizer / UBSan and held to a position-by-position walk written here: contigs, sum of squared lengths, longest contig,
// class, flags, the row of seven sums and the two error counts, for
//   - all 2^16 masks on positions 56 .. 71 (every way a run can meet the 63 / 64 boundary), alone and with a run in front and behind,
//   - every single-run mask [a, b],
//   - 4000 seeded random masks of several densities,
// each at max = 98, 120 and 128 positions and under every setting of SETTINGS (classification off, thresholds 1, 2, 40 and above any
// count, error gates off, fractional and absolute).  The gates of the walk are the general loop's double expressions, not the table's bits.
// Also: gs_sn_shr at every shift, and the max key at read numbers around 2^40.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../genestrip_amd/csrc/gs_snrec.h"

struct Setting {
    int classify, threshold;
    double tax, cls;  // max_read_tax_err, max_read_class_err (< 0: off, < 1: a fraction of max, >= 1: a count)
};
static const Setting SETTINGS[] = {{1, 1, -1, -1}, {1, 2, -1, -1},   {1, 40, -1, -1}, {1, 200, -1, -1}, {0, 1, -1, -1},
                                   {1, 1, 0.1, 0.5}, {1, 3, 0.5, 0.1}, {1, 1, 0.0, 0.0}, {1, 1, 30, 5},   {1, 1, 0.99, -1}};

static long long fails = 0, checked = 0;

// the table as launch_batch builds it
static void build_quot(GsQuotTable &T, int max, double m, double mc) {
    memset(&T, 0, sizeof(T));
    for (int i = 0; i <= max; i++) {
        const double q = (double)i / (double)max;
        T.e[i].q = q;
        T.e[i].q2 = q * q;
        const bool disabled = m >= 0 && ((m >= 1 && (double)i > m) || ((double)i > m * (double)max));
        const bool counted = mc < 0 || (mc >= 1 && (double)i <= mc) || ((double)i <= mc * (double)max);
        if (disabled) T.tax_disabled[i >> 5] |= 1u << (i & 31);
        if (counted) T.class_counted[i >> 5] |= 1u << (i & 31);
    }
}

static void check(uint64_t h0, uint64_t h1, int max, int L, const Setting &s, const GsQuotTable &T) {
    const int vi = 7;
    // the walk: position p is a hit or a miss, a contig is flushed where a hit run ends (or at max: the tail flush)
    uint32_t contigs = 0, sq = 0, longest = 0, kmers = 0, run = 0, miss = 0;
    for (int p = 0; p <= max; p++) {
        const bool hit = p < max && (((p < 64 ? h0 >> p : h1 >> (p - 64)) & 1) != 0);
        if (hit) {
            run++;
            kmers++;
        } else {
            if (p < max) miss++;
            if (run) {
                contigs++;
                sq += run * run;
                if (run > longest) longest = run;
                run = 0;
            }
        }
    }
    int cls = -1, flags = GS_F_FOUND | GS_F_RETURNED, counted = 0;
    const int tax_err = (int)miss;
    int class_err = 0;
    if (s.classify) {
        const bool disabled = s.tax >= 0 && ((s.tax >= 1 && (double)tax_err > s.tax) || ((double)tax_err > s.tax * (double)max));
        if (!disabled) {
            cls = (s.threshold <= 1 || (int)kmers >= s.threshold) ? vi : -1;
            if (cls < 0)
                flags &= ~GS_F_RETURNED;
            else {
                class_err = max - (int)kmers;
                counted = s.cls < 0 || (s.cls >= 1 && (double)class_err <= s.cls) || ((double)class_err <= s.cls * (double)max);
                if (counted) flags |= GS_F_COUNTED;
            }
        }
    }
    uint32_t want[GS_N_SUMS];
    want[GS_S_READS] = (uint32_t)counted;
    want[GS_S_READS_KMERS] = counted ? kmers : 0;
    want[GS_S_KMERS] = kmers;
    want[GS_S_CONTIGS] = contigs;
    want[GS_S_CONTIG_LEN_SQ_SUM] = sq;
    want[GS_S_READS_1KMER] = 1;
    want[GS_S_READS_BPS] = counted ? (uint32_t)L : 0;

    const GsSnConst c = {max, L, s.classify, s.threshold};
    GsSnRow o;
    memset(&o, 0xee, sizeof(o));
    gs_sn_row(h0, h1, vi, c, &T, o);
    checked++;
    bool ok = o.longest == longest && o.out_class == cls && o.out_flags == flags && o.counted == counted;
    for (int i = 0; i < GS_N_SUMS; i++) ok = ok && o.sums[i] == want[i];
    // (the error counts index the quotient table only for a counted read)
    if (counted) ok = ok && o.tax_err == tax_err && o.class_err == class_err;
    if (!ok && fails++ < 10)
        printf("MISMATCH max %d mask %016llx %016llx classify %d threshold %d gates %g %g: contigs %u/%u sq %u/%u longest %u/%u class %d/%d "
               "flags %d/%d counted %d/%d\n",
               max, (unsigned long long)h1, (unsigned long long)h0, s.classify, s.threshold, s.tax, s.cls, o.sums[GS_S_CONTIGS], contigs,
               o.sums[GS_S_CONTIG_LEN_SQ_SUM], sq, o.longest, longest, o.out_class, cls, o.out_flags, flags, o.counted, counted);
}

static uint64_t low(int n) { return n >= 64 ? ~0ULL : (n <= 0 ? 0ULL : (1ULL << n) - 1ULL); }
static void range_mask(int a, int b, uint64_t &h0, uint64_t &h1) {  // positions a .. b
    h0 = low(b + 1) & ~low(a);
    h1 = low(b + 1 - 64) & ~low(a - 64);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

int main() {
    // the shift: every n, against the bit-by-bit definition
    for (int n = 0; n <= 128; n++) {
        const uint64_t a0 = 0x0123456789abcdefULL, a1 = 0xfedcba9876543211ULL;
        uint64_t lo = a0, hi = a1;
        gs_sn_shr(lo, hi, n);
        for (int p = 0; p < 128; p++) {
            const int src = p + n;
            const int want = src < 64 ? (int)((a0 >> src) & 1) : (src < 128 ? (int)((a1 >> (src - 64)) & 1) : 0);
            const int got = p < 64 ? (int)((lo >> p) & 1) : (int)((hi >> (p - 64)) & 1);
            if (got != want && fails++ < 10) printf("MISMATCH shift %d bit %d\n", n, p);
        }
    }
    // the key: the longest contig above bit 40, below it the read number counted down, modulo 2^40
    {
        const uint64_t m40 = (1ULL << 40) - 1;
        const int64_t firsts[] = {0, 1, (1LL << 33) + 5, (1LL << 40) - 3, (1LL << 40), (1LL << 41) + 7};
        const uint32_t reads[] = {0u, 1u, 5u, 4000000000u};
        for (int64_t f : firsts)
            for (uint32_t r : reads) {
                const uint64_t want = (77ULL << 40) | (m40 - ((uint64_t)(f + (int64_t)r) & m40));
                if (gs_sn_max_key(77, f, r) != want && fails++ < 10) printf("MISMATCH key %lld %u\n", (long long)f, r);
            }
    }
    const int maxes[] = {98, 120, 128};
    for (int max : maxes) {
        const int L = max + 30;
        for (const Setting &s : SETTINGS) {
            GsQuotTable T;
            build_quot(T, max, s.tax, s.cls);
            // positions 56 .. 71: alone, and between a run that ends at 40 and one that starts at 80 and reaches max - 1
            for (uint32_t m = 1; m < (1u << 16); m++) {
                const uint64_t h0 = (uint64_t)(m & 0xff) << 56, h1 = (uint64_t)(m >> 8);
                check(h0, h1, max, L, s, T);
                uint64_t f0, f1, b0, b1;
                range_mask(3, 40, f0, f1);
                range_mask(80, max - 1, b0, b1);
                check(h0 | f0 | b0, h1 | f1 | b1, max, L, s, T);
            }
            for (int a = 0; a < max; a++)
                for (int b = a; b < max; b++) {
                    uint64_t h0, h1;
                    range_mask(a, b, h0, h1);
                    check(h0, h1, max, L, s, T);
                }
            rng_state = 1000u + (unsigned)max;
            for (int i = 0; i < 4000; i++) {
                uint64_t h0 = rnd(), h1 = rnd();
                switch (i & 3) {  // half, a quarter, three quarters of the positions, and long runs with a few gaps
                case 1: h0 &= rnd(), h1 &= rnd(); break;
                case 2: h0 |= rnd(), h1 |= rnd(); break;
                case 3: h0 |= rnd() | rnd() | rnd(), h1 |= rnd() | rnd() | rnd(); break;
                }
                h1 &= low(max - 64);
                if ((h0 | h1) == 0) h0 = 1;
                check(h0, h1, max, L, s, T);
            }
        }
    }
    printf("checked %lld records, fails %lld\n", checked, fails);
    return fails ? 1 : 0;
}
