// genomes_emulate.cpp -- the kernels of genestrip_amd/csrc/gs_genomes.hip (genome FASTA text -> regions of the kept records) and the
// block-sum scan of gs_rewrite.hip they use, compiled for the host against a stand-in for the few HIP constructs they use (a block is
// 256 real threads, tests/native/genomes_emulate_hip.h over records_emulate_hip.h) and run under AddressSanitizer / UBSan.  Every array has exactly the size
// the C ABI gives it (gs_api.cpp: gs_genomes_scan / _headers / _gather), so a store or a load outside of it stops the program;
// header lines, bases, offsets, the longest line and the cut must equal those of the host parser (gs_genomeparse.h), and a refused
// chunk must name its first bad byte.
// The test that builds it (tests/test_genomes_native_cpu.py) puts a <hip/hip_runtime.h> that includes genomes_emulate_hip.h on the
// include path.
#include "genomes_emulate_hip.h"
thread_local dim3 threadIdx, blockIdx;
dim3 gridDim;
std::barrier<> *g_block_bar;
std::barrier<> *g_wave_bar[4];
unsigned long long g_xch[4][64];
typedef unsigned long long u64;
#include "../../genestrip_amd/csrc/gs_rewrite.hip"
#include "../../genestrip_amd/csrc/gs_genomes.hip"
#include "../../genestrip_amd/csrc/gs_genomeparse.h"
#include <stdio.h>
#include <random>
#include <string>

static int g_fails = 0;

template <class A, class B>
static bool same(const A &a, const B &b) {
    return a.size() == b.size() && std::equal(a.begin(), a.end(), b.begin());
}

// one chunk through the kernels as gs_api.cpp drives them; keep: one flag per record, or empty = every record.  expect_bad >= 0:
// the chunk must be refused with this offset
static void run(const std::string &name, const std::string &data, bool last, const std::vector<uint8_t> &keep_in, int64_t expect_bad = -1) {
    const int64_t n = (int64_t)data.size(), n_tiles = (n + GS_GN_TILE - 1) / GS_GN_TILE;
    gs_host::GenomeRecords want;
    gs_host::genome_parse((const uint8_t *)data.data(), data.size(), last, &want);
    bool ok = true;
    if (n > 0) {
        std::vector<uint8_t> text((size_t)n_tiles * GS_GN_TILE + GS_GN_PAD, '\n');
        memcpy(text.data(), data.data(), data.size());
        std::vector<u64> tile_hl(n_tiles + 1), tile_c(n_tiles + 1), res(GS_GN_R_WORDS, 0);
        uint32_t status[GS_GN_WORDS] = {0xffffffffu, 0xffffffffu, 0, 0};
        GsGenomesParams P{};
        P.text = text.data();
        P.n_bytes = n;
        P.n_tiles = n_tiles;
        P.last = last;
        P.tile_hl = tile_hl.data();
        P.tile_c = tile_c.data();
        P.status = status;
        P.res = res.data();
        gs_launch_genomes_count(&P, nullptr);
        const uint32_t bad = std::min(status[GS_GN_NUL], status[GS_GN_CR]);
        if (expect_bad >= 0 || bad != 0xffffffffu) {
            ok = (int64_t)bad == expect_bad;
            printf("%s %s\n", name.c_str(), ok ? "ok" : "MISMATCH (refusal)");
            g_fails += !ok;
            return;
        }
        P.n_hdr = (int64_t)(tile_hl[n_tiles] >> 32);
        P.n_nl = (int64_t)(tile_hl[n_tiles] & 0xffffffffu);
        P.n_records = last ? P.n_hdr : std::max<int64_t>(P.n_hdr - 1, 0);
        const int64_t nr = P.n_records, n_blocks = (nr + 255) / 256;
        std::vector<uint32_t> nl(P.n_nl + 1), cnl(P.n_nl + 1), rec_start(P.n_hdr + 1), rec_line(P.n_hdr + 1), base_start(P.n_hdr + 1), base_cnt(P.n_hdr + 1);
        std::vector<u64> hdr_off(nr + 1, 0), sel(nr + 1, 0), off(nr + 1, 0), rec_block(n_blocks + 1, 0);
        P.nl = nl.data();
        P.cnl = cnl.data();
        P.rec_start = rec_start.data();
        P.rec_line = rec_line.data();
        P.base_start = base_start.data();
        P.base_cnt = base_cnt.data();
        P.hdr_off = hdr_off.data();
        P.sel = sel.data();
        P.off = off.data();
        P.rec_block = rec_block.data();
        gs_launch_genomes_records(&P, nullptr);
        std::vector<uint8_t> hdr(res[GS_GN_R_HDR_BYTES]);
        P.hdr_out = hdr.data();
        gs_launch_genomes_headers(&P, nullptr);
        hdr_off.resize(nr + 1);
        ok = ok && (size_t)res[GS_GN_R_CUT] == want.consumed && nr == want.records() && same(hdr, want.headers) && same(hdr_off, want.header_off) &&
             (int64_t)status[GS_GN_MAXLINE] == want.max_line;
        // the regions of the kept records
        std::vector<uint8_t> keep = keep_in;
        keep.resize(nr, 1);
        P.keep = keep_in.empty() ? nullptr : keep.data();
        std::vector<uint8_t> wseq;
        std::vector<u64> woff{0};
        for (int64_t r = 0; r < nr; r++)
            if (keep[r]) {
                wseq.insert(wseq.end(), want.seq.begin() + want.off[r], want.seq.begin() + want.off[r + 1]);
                woff.push_back(wseq.size());
            }
        std::vector<uint8_t> seq;
        if (nr > 0) {
            gs_launch_genomes_select(&P, nullptr);
            const u64 kept = res[GS_GN_R_KEPT];
            seq.assign((size_t)(kept & ((1ULL << 40) - 1)), 0xCC);
            P.seq = seq.data();
            gs_launch_genomes_gather(&P, ((int64_t)res[GS_GN_R_CUT] + GS_GN_TILE - 1) / GS_GN_TILE, nullptr);
            off.resize((size_t)(kept >> 40) + 1);
        } else {
            off.assign(1, 0);
        }
        ok = ok && same(seq, wseq) && same(off, woff);
    } else {
        ok = want.records() == 0;
    }
    printf("%s %s\n", name.c_str(), ok ? "ok" : "MISMATCH");
    g_fails += !ok;
}

static std::string bases(std::mt19937_64 &rng, size_t n) {
    std::string s(n, ' ');
    for (auto &c : s) c = "ACGT"[rng() % 4];
    return s;
}

int main() {
    std::mt19937_64 rng(3);
    const std::vector<uint8_t> all;
    // the hand-written streams (tests/genomefasta_cases.py)
    const char *hand[] = {">a\nAC\nGT\n", ">a\r\nAC\r\nGT\r\n", ">a\nAC\r\r\n", ">a\nA\rC\n", ">a\nA\r\rC\r\n", ">a\nAC\n\nGT\n\r\n", ">a\n\r\nAC\n",
                          ">a\n>b\nAC\n>c\n", "ACGT\n\n>a\nGG\n", ">a\nAC\nGT", ">a\nAC\nGT\r", ">a\nAC\n>b", ">a\nAC>GT\n", ">a\nacgtN\n",
                          ">a\nAC\n>b\nGG\n", ">a\nAC\n\n>b x\nGG\nT", ">a\nAC\n", "AC\nGT", "ACGT", ""};
    for (size_t i = 0; i < sizeof(hand) / sizeof(hand[0]); i++)
        for (int last = 0; last < 2; last++) run(std::string("hand ") + (last ? "last " : "more ") + std::to_string(i), hand[i], last != 0, all);

    // line lengths around a thread's 16 bytes and a wave's 64, behind headers of every length; LF and CRLF
    for (const char *eol : {"\n", "\r\n"}) {
        std::string data;
        int n_rec = 0;
        for (int hl = 1; hl <= 17; hl++)
            for (int L : {0, 1, 15, 16, 17, 63, 64, 65}) {
                data += ">" + std::string(hl - 1, 'h') + eol;
                for (int l = 0; l < 3; l++) data += bases(rng, L) + eol;
                n_rec++;
            }
        run(std::string("line lengths ") + (eol[0] == '\n' ? "LF" : "CRLF"), data, true, all);
        std::vector<uint8_t> keep(n_rec);
        for (int i = 0; i < n_rec; i++) keep[i] = i % 3 != 1;
        run(std::string("line lengths, two of three kept ") + (eol[0] == '\n' ? "LF" : "CRLF"), data, true, keep);
        run(std::string("line lengths, not the last chunk ") + (eol[0] == '\n' ? "LF" : "CRLF"), data.substr(0, data.size() - 3), false, keep);
    }

    // unwrapped records around one piece of the gather, two pieces and a half, kept and skipped by turns
    for (int n : {GS_GN_TILE - 1, GS_GN_TILE, GS_GN_TILE + 1, 2 * GS_GN_TILE + 2048}) {
        std::string data;
        for (int i = 0; i < 3; i++) data += ">u" + std::to_string(i) + "\n" + bases(rng, n - 1) + "\n";
        data += ">tail\n" + bases(rng, n - 1);
        run("unwrapped " + std::to_string(n), data, true, all);
        run("unwrapped " + std::to_string(n) + " 0101", data, true, {0, 1, 0, 1});
        run("unwrapped " + std::to_string(n) + " 1010", data, true, {1, 0, 1, 0});
        run("unwrapped " + std::to_string(n) + " cut", data.substr(0, data.size() - 5), false, all);
    }

    // an empty record kept between two long ones; none kept; only the first; only the last
    {
        const std::string data = ">long one\n" + bases(rng, 3 * GS_GN_TILE + 5) + "\n>empty\n>long two\n" + bases(rng, 2 * GS_GN_TILE + 9) + "\n";
        for (int m : {2, 3, 5, 6, 7}) run("empty between long ones, mask " + std::to_string(m), data, true, {(uint8_t)(m & 1), (uint8_t)(m >> 1 & 1), (uint8_t)(m >> 2 & 1)});
    }

    // terminators and header lines across the edges of a thread's bytes and of a tile
    for (int edge : {16, GS_GN_TILE, 2 * GS_GN_TILE})
        for (const char *tail : {"\r\nAC\n", "\rC\nAC\n", "\n>next\nAC\n", "\r\r\r\nAC\n", "\r\r\rG\n"})
            for (int shift = 0; shift < 3; shift++) {
                const std::string data = ">e\n" + bases(rng, edge - 3 - 1 + shift - 1) + tail + ">z\n" + bases(rng, 40) + "\r";
                run("edge " + std::to_string(edge) + " shift " + std::to_string(shift), data, true, all);
                if (shift == 1) run("edge " + std::to_string(edge) + " shift " + std::to_string(shift) + " more", data, false, all);
            }

    // more than 256 records (the scans over records cross a block), short ones
    {
        const char *pool[] = {">\nA\n", ">ab\n", ">x\nAC\nG\n", ">yy\r\nT\r\n"};
        std::string data;
        std::vector<uint8_t> keep;
        for (int i = 0; i < 700; i++) {
            data += pool[(i * 7 + i / 5) % 4];
            keep.push_back(i % 2 == 0);
        }
        run("700 short records", data, true, all);
        run("700 short records, alternating", data, true, keep);
    }

    // random streams of every line shape
    for (int round = 0; round < 6; round++) {
        std::string data = round % 2 ? "" : "AC\n\r\n";
        const int n_rec = 1 + (int)(rng() % 30);
        std::vector<uint8_t> keep;
        for (int i = 0; i < n_rec; i++) {
            const char *eol = rng() % 3 ? "\n" : "\r\n";
            data += ">r" + std::to_string(i) + std::string(rng() % 20, 'y') + eol;
            const int lines = (int)(rng() % 6);
            for (int l = 0; l < lines; l++) {
                const int len = (int)(rng() % 200);
                for (int j = 0; j < len; j++) data += "ACGT\r>"[rng() % 64 < 60 ? rng() % 4 : 4 + rng() % 2];
                data += eol;
            }
        }
        if (round % 3 == 0) data += "ACG\r";
        gs_host::GenomeRecords w;
        gs_host::genome_parse((const uint8_t *)data.data(), data.size(), true, &w);
        for (int64_t i = 0; i < w.records(); i++) keep.push_back(rng() % 2);
        run("random " + std::to_string(round), data, true, keep);
        run("random " + std::to_string(round) + " more", data, false, all);
    }

    // refusals: the first NUL byte; a run of '\r' of the cap is taken, one more is refused with the offset of the run's first byte
    {
        std::string good = ">c\nAC" + std::string(GS_GN_CR_CAP, '\r') + "GT\nAA" + std::string(GS_GN_CR_CAP, '\r') + "\n>d\nTT" + std::string(GS_GN_CR_CAP, '\r');
        run("runs of the cap", good, true, all);
        std::string nul = ">a\n" + bases(rng, 5000) + "\n";
        nul[4500] = 0;
        nul[4700] = 0;
        run("NUL", nul, true, all, 4500);
        run("run over the cap", ">c\nAC" + std::string(GS_GN_CR_CAP + 1, '\r') + "GT\n", true, all, 5);
        run("run over the cap across a tile", ">c\n" + bases(rng, GS_GN_TILE - 30) + std::string(GS_GN_CR_CAP + 1, '\r') + "\n>d\n", true, all, 3 + GS_GN_TILE - 30);
        run("a long run at the end", ">c\nAC\n" + std::string(300, '\r'), true, all, 6);
    }
    printf("fails %d\n", g_fails);
    return g_fails != 0;
}
