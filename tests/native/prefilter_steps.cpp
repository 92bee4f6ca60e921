// The two host-checkable halves of gs_pf_kernel (genestrip_amd/csrc/gs_prefilter.h), compiled for the host under AddressSanitizer / UBSan:
//   prefilter_steps decide <case file>   the grouped decision (gs_pf_group_l1, gs_pf_group_decide) run the way the kernel runs it --
//        sample 0, then groups of GS_PF_GROUP samples (gs_pf_group_size), a short group filled up with its last sample and masked,
//        the codes by gs_pf_canon15_dot (held to gs_pf_canon15 for every sample) -- agrees with gs_pf_read_passes
//        for every read of the case file (the format of prefilter_emulate.cpp), the deciding sample is the first one gs_pf_sample_in
//        accepts, the exact level is never asked for a sample whose level-one bit is clear and never twice for one sample
//   prefilter_steps copy                  the copy's index arithmetic (gs_pf_copy_pieces, gs_pf_piece_range, gs_pf_wave_bytes) for every
//        base alignment 0 .. 15, every number of reads 1 .. 64 of a wave round, every L from 32 to 158 and every position
//        of the round in the batch: the pieces tile the round's bytes without a gap, lie inside the wave's buffer, touch no byte in
//        front of the batch's first or behind its last read, piece 1 is whole (the load of a lane that has no piece of its own),
//        the samples' dword reads stay inside the buffer, and a copy made piece by piece from a source of exactly nr L bytes puts
//        every byte of every read where the lanes look for it
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../genestrip_amd/csrc/gs_prefilter.h"

template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static void sample_dwords(const uint8_t *p, uint32_t *d) {
    d[0] = d[1] = d[2] = d[3] = 0;
    for (int j = 0; j < GS_MIN_L; j++) d[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
}

static int run_decide(const char *path) {
    FILE *f = fopen(path, "rb");
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
    if (!ok || gs_pf_samples(L, k) != m) return 2;
    std::vector<uint32_t> l1((size_t)1 << (GS_PF_L1_BITS - 5), 0u), l2(GS_PF_L2_WORDS, 0u);
    for (int64_t c : set) {
        l2[(size_t)c >> 5] |= 1u << (c & 31);
        const uint32_t b = gs_pf_l1_bit((uint32_t)c);
        l1[b >> 5] |= 1u << (b & 31);
    }
    const int w = gs_pf_stride(k);
    int fails = 0, n_pass = 0;
    long asked_total = 0, asked_not_in_s = 0, deciders[64] = {0};
    for (int r = 0; r < n && fails < 20; r++) {
        const uint8_t *rd = reads[r].data();
        // what gs_pf_read_passes does, sample by sample: the first sample it accepts
        int want = -1;
        for (int i = 0; i < m && want < 0; i++) {
            uint32_t d[4];
            sample_dwords(rd + i * w, d);
            if (gs_pf_sample_in(l1.data(), l2.data(), d[0], d[1], d[2], d[3])) want = i;
        }
        if ((want >= 0) != gs_pf_read_passes(l1.data(), l2.data(), rd, L, k) || (want >= 0) != (pass[r] != 0)) {
            printf("MISMATCH read %d: the sample walk, gs_pf_read_passes and the restatement disagree\n", r);
            fails++;
        }
        // the kernel's way
        std::vector<int> asked((size_t)m, 0);
        int got = -1;
        for (int s0 = 0, ng = 0; s0 < m && got < 0; s0 += ng) {
            ng = gs_pf_group_size(s0, m);
            uint32_t codes[GS_PF_GROUP], l1w[GS_PF_GROUP];
            for (int i = 0; i < GS_PF_GROUP; i++) {
                uint32_t d[4];
                sample_dwords(rd + (s0 + (i < ng ? i : ng - 1)) * w, d);
                codes[i] = gs_pf_canon15_dot(d[0], d[1], d[2], d[3]);
                if (codes[i] != gs_pf_canon15(d[0], d[1], d[2], d[3])) {  // (every byte value: the case files hold N, lower case, CR)
                    printf("MISMATCH read %d sample %d: gs_pf_canon15_dot %u, gs_pf_canon15 %u\n", r, s0 + i, codes[i], gs_pf_canon15(d[0], d[1], d[2], d[3]));
                    fails++;
                }
                l1w[i] = l1[gs_pf_l1_bit(codes[i]) >> 5];
            }
            const uint32_t todo = gs_pf_group_l1(codes, l1w, GS_PF_GROUP) & ((1u << ng) - 1u);
            const int dec = gs_pf_group_decide(todo, [&](int i) {
                const int s = s0 + i;
                if (i < 0 || i >= ng) {
                    printf("MISMATCH read %d: sample %d of a group of %d asked for\n", r, i, ng);
                    fails++;
                    return false;
                }
                asked[(size_t)s]++;
                asked_total++;
                const uint32_t c = codes[i], b = gs_pf_l1_bit(c);
                if (((l1[b >> 5] >> (b & 31)) & 1u) == 0) {
                    printf("MISMATCH read %d sample %d: the exact level asked though level one is clear\n", r, s);
                    fails++;
                }
                if (((l2[c >> 5] >> (c & 31)) & 1u) == 0) {
                    asked_not_in_s++;
                    return false;
                }
                uint32_t d[4];
                sample_dwords(rd + s * w, d);
                return gs_pf_bad15(d[0], d[1], d[2], d[3]) == 0;
            });
            if (dec >= 0) got = s0 + dec;
        }
        for (int i = 0; i < m; i++)
            if (asked[(size_t)i] > 1 || (got >= 0 && i > got && asked[(size_t)i])) {
                printf("MISMATCH read %d sample %d: asked %d times (decided by %d)\n", r, i, asked[(size_t)i], got);
                fails++;
            }
        if (got != want) {
            printf("MISMATCH read %d: decided by sample %d, gs_pf_sample_in accepts %d first\n", r, got, want);
            fails++;
        }
        if (got >= 0) {
            n_pass++;
            deciders[got < 63 ? got : 63]++;
        }
    }
    printf("k %d L %d m %d: %d reads, %d pass, exact level asked %ld times, %ld of them not in S, fails %d\ndeciding sample:", k, L, m, n,
           n_pass, asked_total, asked_not_in_s, fails);
    for (int i = 0; i < m && i < 64; i++) printf(" %ld", deciders[i]);
    printf("\n");
    if (!fails) printf("case ok\n");
    return fails ? 1 : 0;
}

static int copy_fails = 0;
static void copy_fail(const char *what, int delta, int nr, int L, int first, int last, int c) {
    if (copy_fails++ < 20) printf("MISMATCH %s: delta %d nr %d L %d first %d last %d piece %d\n", what, delta, nr, L, first, last, c);
}

static int run_copy() {
    long combos = 0, pieces_seen = 0, copies = 0;
    for (int L = 32; L <= 31 + 127; L++) {  // (32 = the shortest read gs_launch_prefilter takes; the library sends 128 .. k + 127)
        const int room = (int)gs_pf_wave_bytes(L);
        for (int nr = 1; nr <= 64; nr++)
            for (int delta = 0; delta < 16; delta++) {
                const int end = delta + nr * L, pieces = gs_pf_copy_pieces(delta, nr, L);
                if (16 * pieces < end || 16 * (pieces - 1) >= end) copy_fail("number of pieces", delta, nr, L, 0, 0, pieces);
                for (int first = 0; first < 2; first++)
                    for (int last = 0; last < 2; last++) {
                        combos++;
                        int at = first ? delta : 0;  // the pieces follow one another without a gap from here
                        for (int c = 0; c < pieces; c++) {
                            int lo = -1, hi = -1;
                            gs_pf_piece_range(c, delta, nr, L, first != 0, last != 0, &lo, &hi);
                            pieces_seen++;
                            if (lo != at || hi <= lo || hi - lo > 16) copy_fail("gap, overlap or empty piece", delta, nr, L, first, last, c);
                            if (lo < 16 * c || hi > 16 * c + 16 || 16 * c + 16 > room) copy_fail("outside the piece's place or the buffer", delta, nr, L, first, last, c);
                            if (first && lo < delta) copy_fail("in front of the batch", delta, nr, L, first, last, c);
                            if (last && hi > end) copy_fail("behind the batch", delta, nr, L, first, last, c);
                            if ((hi - lo == 16) != ((!first || 16 * c >= delta) && (!last || 16 * c + 16 <= end)))
                                copy_fail("whole", delta, nr, L, first, last, c);
                            at = hi;
                        }
                        if (at < end || (last && at != end)) copy_fail("the round's bytes are not covered", delta, nr, L, first, last, pieces);
                        int lo = 0, hi = 0;  // a lane without a piece of its own loads piece 1
                        gs_pf_piece_range(1, delta, nr, L, first != 0, last != 0, &lo, &hi);
                        if (pieces < 2 || lo != 16 || hi != 32) copy_fail("piece 1 is not whole", delta, nr, L, first, last, 1);
                    }
                // the dwords a lane reads for its last sample (five from (b >> 2) on) stay inside the buffer, at every k with this L
                for (int k = GS_MIN_K; k <= 31; k++) {
                    if (L < k + 64 || L > k + 127) continue;
                    const int b = delta + (nr - 1) * L + (gs_pf_samples(L, k) - 1) * gs_pf_stride(k);
                    if (b + GS_MIN_L > end || 4 * (b >> 2) + 20 > room) copy_fail("sample read outside the buffer", delta, nr, L, k, 0, -1);
                }
                // the copy itself, the round being the whole batch: a source of exactly nr L bytes, whole pieces as 16 bytes, cut
                // ones byte by byte, every lane's pieces lane, lane + 64, ..
                if (!(nr <= 2 || nr >= 63 || L == 83 || L == 150 || L == 151 || L == 158)) continue;
                copies++;
                std::vector<uint8_t> src((size_t)nr * L), buf((size_t)room, 0xEE);
                for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)(i * 131u + (i >> 8) + 7u);
                for (int lane = 0; lane < 64; lane++)
                    for (int c = lane; c < pieces; c += 64) {
                        int lo = 0, hi = 0;
                        gs_pf_piece_range(c, delta, nr, L, true, true, &lo, &hi);
                        if (hi - lo == 16)
                            memcpy(buf.data() + 16 * c, src.data() + (16 * c - delta), 16);
                        else
                            for (int b = lo; b < hi; b++) buf.at((size_t)b) = src.at((size_t)(b - delta));
                    }
                if (memcmp(buf.data() + delta, src.data(), src.size()) != 0) copy_fail("copied bytes", delta, nr, L, 1, 1, -1);
            }
    }
    printf("copy: %ld rounds, %ld pieces, %ld copies, fails %d\n", combos, pieces_seen, copies, copy_fails);
    if (!copy_fails) printf("copy ok\n");
    return copy_fails ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "decide")) return run_decide(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "copy")) return run_copy();
    return 2;
}
