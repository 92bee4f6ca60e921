// genomeparse_sanitize.cpp -- genestrip_amd/csrc/gs_genomeparse.h (the line-by-line genome FASTA parser of the host layer) on its
// own under AddressSanitizer / UBSan, held to the hand-written streams of tests/genomefasta_cases.py (the answers are worked out
// from the reference's Java there) and, on random streams of every line shape, to a walk in chunks of every size.
#include "../../genestrip_amd/csrc/gs_genomeparse.h"

#include <stdio.h>

#include <random>
#include <string>

using gs_host::GenomeRecords;

static int g_fails = 0;

struct Case {
    const char *name;
    std::string data;
    bool last;
    std::vector<std::string> headers;
    std::string seq;
    std::vector<uint64_t> off;
    int64_t max_line;
    size_t consumed;
};

static std::string S(const char *s, size_t n) { return std::string(s, n); }
#define LIT(s) S(s, sizeof(s) - 1)

static void check(const Case &c) {
    GenomeRecords r;
    gs_host::genome_parse((const uint8_t *)c.data.data(), c.data.size(), c.last, &r);
    std::string hdr;
    std::vector<uint64_t> hoff{0};
    for (auto &h : c.headers) {
        hdr += h;
        hoff.push_back(hdr.size());
    }
    const bool ok = std::string(r.headers.begin(), r.headers.end()) == hdr && r.header_off == hoff && std::string(r.seq.begin(), r.seq.end()) == c.seq &&
                    r.off == c.off && r.max_line == c.max_line && r.consumed == c.consumed;
    printf("%s %s\n", c.name, ok ? "ok" : "MISMATCH");
    g_fails += !ok;
}

int main() {
    const std::vector<Case> cases = {
        {"LF", LIT(">a\nAC\nGT\n"), true, {">a"}, "ACGT", {0, 4}, 3, 9},
        {"CRLF", LIT(">a\r\nAC\r\nGT\r\n"), true, {">a\r"}, "ACGT", {0, 4}, 4, 12},
        {"two CR", LIT(">a\nAC\r\r\n"), true, {">a"}, "AC", {0, 2}, 5, 8},
        {"CR inside a line", LIT(">a\nA\rC\n"), true, {">a"}, "A\rC", {0, 3}, 4, 7},
        {"CR run inside a line", LIT(">a\nA\r\rC\r\n"), true, {">a"}, "A\r\rC", {0, 4}, 6, 9},
        {"empty lines", LIT(">a\nAC\n\nGT\n\r\n"), true, {">a"}, "ACGT", {0, 4}, 3, 12},
        {"a line of one CR", LIT(">a\n\r\nAC\n"), true, {">a"}, "AC", {0, 2}, 3, 8},
        {"header-only records", LIT(">a\n>b\nAC\n>c\n"), true, {">a", ">b", ">c"}, "AC", {0, 0, 2, 2}, 3, 12},
        {"data in front of the first header", LIT("ACGT\n\n>a\nGG\n"), true, {">a"}, "GG", {0, 2}, 5, 12},
        {"no final newline", LIT(">a\nAC\nGT"), true, {">a"}, "ACGT", {0, 4}, 3, 8},
        {"final bare CR", LIT(">a\nAC\nGT\r"), true, {">a"}, "ACGT", {0, 4}, 3, 9},
        {"final header without newline", LIT(">a\nAC\n>b"), true, {">a", ">b"}, "AC", {0, 2, 2}, 3, 8},
        {"'>' inside a data line", LIT(">a\nAC>GT\n"), true, {">a"}, "AC>GT", {0, 5}, 6, 9},
        {"lower case stays", LIT(">a\nacgtN\n"), true, {">a"}, "acgtN", {0, 5}, 6, 9},
        {"NUL byte", LIT(">a\nA\0C\n"), true, {">a"}, "AC", {0, 2}, 3, 7},
        {"NUL bytes alone at the end", LIT(">a\nAC\n\0\0"), true, {">a"}, "AC", {0, 2}, 3, 8},
        {"empty stream", "", true, {}, "", {0}, 0, 0},
        {"cut behind a newline", LIT(">a\nAC\n>b\nGG\n"), false, {">a"}, "AC", {0, 2}, 3, 6},
        {"cut inside a header line", LIT(">a\nAC\n>b"), false, {">a"}, "AC", {0, 2}, 3, 6},
        {"cut inside a data line", LIT(">a\nAC\n\n>b x\nGG\nT"), false, {">a"}, "AC", {0, 2}, 3, 7},
        {"one header only", LIT(">a\nAC\n"), false, {}, "", {0}, 0, 0},
        {"no header at all", LIT("AC\nGT"), false, {}, "", {0}, 3, 3},
        {"no header, no newline", LIT("ACGT"), false, {}, "", {0}, 0, 0},
    };
    for (auto &c : cases) check(c);

    // a random stream walked whole and in chunks of every size: the rest behind `consumed` goes in front of the next block
    std::mt19937_64 rng(5);
    for (int round = 0; round < 20; round++) {
        std::string stream = round % 2 ? "" : "AC\n\r\n";
        const int n_rec = 1 + (int)(rng() % 12);
        for (int i = 0; i < n_rec; i++) {
            const char *eol = rng() % 3 ? "\n" : "\r\n";
            stream += ">r" + std::to_string(i) + eol;
            const int lines = (int)(rng() % 5);
            for (int l = 0; l < lines; l++) {
                const int len = (int)(rng() % 40);
                for (int j = 0; j < len; j++) stream += "ACGT\r>"[rng() % 64 < 60 ? rng() % 4 : 4 + rng() % 2];  // (a '>' may open a line: a header line then)
                stream += eol;
            }
        }
        if (round % 3 == 0) stream += "ACG";
        GenomeRecords whole;
        gs_host::genome_parse((const uint8_t *)stream.data(), stream.size(), true, &whole);
        for (size_t block : {(size_t)1, (size_t)3, (size_t)16, (size_t)50, stream.size() + 1}) {
            std::vector<uint8_t> hdr, seq;
            std::vector<uint64_t> hoff{0}, off{0};
            int64_t max_line = 0;
            std::string rest;
            size_t pos = 0;
            for (;;) {
                const std::string take = stream.substr(pos, block);
                pos += take.size();
                const std::string chunk = rest + take;
                const bool last = pos >= stream.size();
                GenomeRecords r;
                gs_host::genome_parse((const uint8_t *)chunk.data(), chunk.size(), last, &r);
                hdr.insert(hdr.end(), r.headers.begin(), r.headers.end());
                seq.insert(seq.end(), r.seq.begin(), r.seq.end());
                for (size_t i = 1; i < r.off.size(); i++) {
                    off.push_back((seq.size() - r.seq.size()) + r.off[i]);
                    hoff.push_back((hdr.size() - r.headers.size()) + r.header_off[i]);
                }
                if (r.max_line > max_line) max_line = r.max_line;
                rest = chunk.substr(r.consumed);
                if (last) break;
            }
            const bool ok = hdr == whole.headers && seq == whole.seq && hoff == whole.header_off && off == whole.off && max_line == whole.max_line;
            printf("round %d block %zu %s\n", round, block, ok ? "ok" : "MISMATCH");
            g_fails += !ok;
        }
    }
    printf("fails %d\n", g_fails);
    return g_fails != 0;
}
