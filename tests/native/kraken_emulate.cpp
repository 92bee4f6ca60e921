// kraken_emulate.cpp -- the text kernels of genestrip_amd/csrc/gs_kraken.hip (sizes, offsets, the lines through the LDS tile, the
// block-wide long line) compiled for the host against a stand-in for the few HIP constructs they use -- a block is 256 real
// threads, a wave 64 of them, ballot / shuffle / barrier are exchanges through memory -- and run under AddressSanitizer / UBSan on
// random chunks: the text must equal a straightforward formatter's byte for byte, and the 16 bytes in front of the output and
// behind it (which a block shares with nothing) must stay untouched.  Names of kilobytes, reads of thousands of segments, blocks
// whose lines span several tiles, k = 2 and k = 31, write_all on and off, a chunk of one read.
// The test that builds it (tests/test_krakenlines_cpu.py) puts a <hip/hip_runtime.h> that includes kraken_emulate_hip.h on the include path.
#include "kraken_emulate_hip.h"
thread_local dim3 threadIdx, blockIdx;
dim3 gridDim;
std::barrier<> *g_block_bar;
std::barrier<> *g_wave_bar[4];
unsigned long long g_xch[4][64];
typedef unsigned long long u64;
extern "C" hipError_t gs_launch_scan_blocks(u64 *blocks, int64_t n_blocks, u64 *total_out, hipStream_t) {
    u64 run = 0;
    for (int64_t i = 0; i < n_blocks; i++) { u64 c = blocks[i]; blocks[i] = run; run += c; }
    *total_out = run;
    return 0;
}
#include "../../genestrip_amd/csrc/gs_kraken.hip"
#include <random>
#include <string>
#include <stdio.h>
int main(int argc, char **argv) {
    int fails = 0;
    for (int seed = 1; seed <= 8; seed++) {
        std::mt19937_64 rng(seed);
        const int k = seed % 2 ? 2 : 31;
        const int64_t n = (seed == 3) ? 1 : 300 + (rng() % 600);
        std::vector<std::string> tax = {"", "5", "1234567", std::string(40, 'x')};
        std::string text; std::vector<uint32_t> nl; std::vector<int32_t> cls, code, start; std::vector<u64> soff{0};
        std::string want; u64 want_lines = 0;
        const int write_all = seed != 4;
        for (int64_t r = 0; r < n; r++) {
            // descriptor
            size_t dl = rng() % 40; if (rng() % 50 == 0) dl = 250 + rng() % 3000; if (rng() % 20 == 0) dl = rng() % 2; if (seed >= 7) dl = 200 + rng() % 49;
            std::string d;
            for (size_t i = 0; i < dl; i++) d += (char)(i == 0 ? '@' : (rng() % 12 == 0 && seed < 7 ? ' ' : 'a' + rng() % 26));
            uint32_t L = 1 + rng() % 400; if (rng() % 100 == 0) L = 3000 + rng() % 40000;
            text += d; nl.push_back(text.size()); text += '\n';
            text += std::string(L, 'C'); nl.push_back(text.size()); text += '\n';
            text += "+"; nl.push_back(text.size()); text += '\n';
            text += std::string(L, 'I'); nl.push_back(text.size()); text += '\n';
            int64_t maxp = (int64_t)L - k + 1;
            int32_t cl = (int32_t)(rng() % 5) - 1;  // -1 .. 3
            cls.push_back(cl);
            // segments: random cut of [0, maxp)
            std::vector<std::pair<int32_t, int32_t>> segs;
            if (maxp > 0) {
                int32_t p = 0;
                while (p < maxp) {
                    int32_t len = 1 + rng() % (rng() % 4 == 0 ? 2 : (rng() % 3 ? 12 : 1200));
                    if (p + len > maxp) len = maxp - p;
                    segs.push_back({(int32_t)(rng() % 6) - 2, p});
                    p += len;
                }
            }
            for (auto &s : segs) { code.push_back(s.first); start.push_back(s.second); }
            soff.push_back(soff.back() + segs.size());
            if (segs.empty() || !(write_all || cl >= 0)) continue;
            want_lines++;
            want += cl >= 0 ? "C\t" : "U\t";
            if (d.size() > 1) { size_t sp = d.find(' ', 1); want += d.substr(1, sp == std::string::npos ? std::string::npos : sp - 1); }
            want += '\t'; want += cl >= 0 ? tax[cl] : "0"; want += '\t'; want += std::to_string(L); want += '\t';
            for (size_t i = 0; i < segs.size(); i++) {
                if (i) want += ' ';
                int32_t c = segs[i].first;
                want += c == -2 ? "A" : c < 0 ? "0" : tax[c];
                want += ':';
                want += std::to_string((i + 1 < segs.size() ? segs[i + 1].second : maxp) - segs[i].second);
            }
            want += '\n';
        }
        std::vector<uint8_t> tb; std::vector<uint32_t> toff{0};
        for (auto &t : tax) { tb.insert(tb.end(), t.begin(), t.end()); toff.push_back(tb.size()); }
        tb.push_back(0);
        std::vector<uint32_t> name_len(n); std::vector<u64> rec(n + 1), blocks((n + 255) / 256 + 1); u64 totals[2] = {0, 0};
        GsKrakenParams P{};
        P.text = (const uint8_t *)text.data(); P.nl = nl.data(); P.n_reads = n; P.k = k; P.write_all = write_all; P.cls = cls.data();
        P.seg_off = soff.data(); P.seg_code = code.data(); P.seg_start = start.data(); P.tax_bytes = tb.data(); P.tax_off = toff.data();
        P.name_len = name_len.data(); P.rec_out = rec.data(); P.rec_block = blocks.data(); P.totals = totals;
        gs_launch_kraken_size(&P, nullptr);
        // guard bytes around the output: nothing may be written outside [0, total)
        std::vector<uint8_t> outbuf(totals[0] + 64 + 16, 0xEE);
        // keep the 16-byte alignment of the text's first byte
        uint8_t *base = outbuf.data(); while (((uintptr_t)base & 15) != 0) base++; base += 16;
        P.out = base;
        if (totals[0]) gs_launch_kraken_write(&P, nullptr);
        bool ok = totals[0] == want.size() && totals[1] == want_lines && memcmp(base, want.data(), want.size()) == 0;
        for (int i = 1; i <= 16; i++) ok = ok && base[-i] == 0xEE;
        for (int i = 0; i < 16; i++) ok = ok && base[totals[0] + i] == 0xEE;
        printf("seed %d k %d n %lld: bytes %llu (want %zu) lines %llu (want %llu) %s\n", seed, k, (long long)n, totals[0], want.size(), totals[1], want_lines, ok ? "ok" : "MISMATCH");
        if (!ok) {
            fails++;
            size_t i = 0; while (i < want.size() && i < totals[0] && base[i] == (uint8_t)want[i]) i++;
            printf("  first difference at byte %zu: got '%.60s' want '%.60s'\n", i, (const char *)base + (i > 20 ? i - 20 : 0), want.c_str() + (i > 20 ? i - 20 : 0));
        }
    }
    printf("fails %d\n", fails);
    return fails != 0;
}
