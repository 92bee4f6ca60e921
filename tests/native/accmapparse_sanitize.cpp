// The line-by-line accession map parser of the host layer (genestrip_amd/csrc/gs_accmapparse.h) on its own under AddressSanitizer /
// UBSan.  It reads the cases tests/test_accmap_native_cpu.py writes out of tests/accmap_cases.py (the hand-worked ones and generated
// text), prints what the parser makes of each -- the test compares that with the expected values and with tests/accmap.py -- and
// checks on its own that every split of a text into two feeds of whole lines gives what one feed gives, and that the index answers
// every key with its first entry.
//
// The case file: n_cases, then per case the lines `dna rna mrna`, `n_cat` and that many category lines, `n_stat` and that many status
// lines, `n_known` and one line of tax ids, `n_bytes`, and n_bytes of catalog text followed by a newline.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../genestrip_amd/csrc/gs_accmapparse.h"

using gs_host::AccmapExact;
using gs_host::AccmapIndex;

static int fails = 0;
#define CHECK(c)                                          \
    do {                                                  \
        if (!(c)) {                                       \
            fails++;                                      \
            printf("FAILED line %d: %s\n", __LINE__, #c); \
        }                                                 \
    } while (0)

static std::string read_line(FILE *f) {
    std::string s;
    int c;
    while ((c = fgetc(f)) != EOF && c != '\n') s.push_back((char)c);
    return s;
}

static bool feed(AccmapExact &k, const std::string &s, bool last) {
    // (a copy of exactly the bytes, so that a read past either end is a heap overflow the sanitizer sees)
    std::vector<uint8_t> b(s.begin(), s.end());
    return k.feed(b.data(), b.size(), last);
}

static bool same(const AccmapExact &a, const AccmapExact &b) {
    if (a.passing != b.passing || a.lines != b.lines || a.line_no != b.line_no || a.entries.size() != b.entries.size()) return false;
    for (size_t i = 0; i < a.entries.size(); i++)
        if (a.entries[i].key != b.entries[i].key || a.entries[i].node != b.entries[i].node) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int n_cases = atoi(read_line(f).c_str());
    for (int c = 0; c < n_cases; c++) {
        AccmapExact proto;
        int dna = 0, rna = 0, mrna = 0;
        sscanf(read_line(f).c_str(), "%d %d %d", &dna, &rna, &mrna);
        proto.dna = dna;
        proto.rna = rna;
        proto.mrna = mrna;
        for (int i = atoi(read_line(f).c_str()); i > 0; i--) proto.categories.push_back(read_line(f));
        for (int i = atoi(read_line(f).c_str()); i > 0; i--) proto.statuses.push_back(read_line(f));
        const int n_known = atoi(read_line(f).c_str());
        {
            const std::string ids = read_line(f);
            const char *p = ids.c_str();
            for (int i = 0; i < n_known; i++) proto.known.push_back((int32_t)strtol(p, (char **)&p, 10));
        }
        const size_t n_bytes = (size_t)atoll(read_line(f).c_str());
        std::string text(n_bytes, '\0');
        CHECK(fread(&text[0], 1, n_bytes, f) == n_bytes);
        read_line(f);

        AccmapExact whole = proto;
        if (!feed(whole, text, true)) {
            CHECK(!whole.error.empty());
            printf("case %d throws %lld\n", c, (long long)whole.line_no);
            continue;
        }
        printf("case %d ok %lld %lld %zu\n", c, (long long)whole.passing, (long long)whole.lines, whole.entries.size());
        for (const auto &e : whole.entries) {
            printf("  ");
            for (unsigned char b : e.key) printf("%02x", b);
            printf(" %d\n", e.node);
        }
        // two feeds (the buffer lives across them); at most 64 cuts of a long text
        size_t cuts = 0;
        for (size_t cut = 1; cut <= text.size() && cuts < 64; cut++) {
            if (text[cut - 1] != '\n') continue;
            cuts++;
            AccmapExact k = proto;
            CHECK(feed(k, text.substr(0, cut), false) && feed(k, text.substr(cut), true));
            CHECK(same(k, whole));
            // a first part that another judge took (the device: lines without NUL, none above the buffer) leaves the same bytes behind
            const std::string head = text.substr(0, cut);
            bool plain = head.find('\0') == std::string::npos;
            for (size_t a = 0, b; plain && a < head.size(); a = b + 1) plain = (b = head.find('\n', a)) - a + 1 <= 2048;
            if (!plain) continue;
            AccmapExact fed = proto, noted = proto;
            CHECK(feed(fed, head, false));
            const size_t e0 = fed.entries.size();
            const long long p0 = fed.passing;
            std::vector<uint8_t> hb(head.begin(), head.end());
            noted.note_chunk(hb.data(), hb.size());
            const bool a_ok = feed(fed, text.substr(cut), true), b_ok = feed(noted, text.substr(cut), true);
            CHECK(a_ok == b_ok);
            if (!a_ok) continue;
            CHECK(fed.passing - p0 == noted.passing && fed.entries.size() - e0 == noted.entries.size());
            for (size_t i = 0; i < noted.entries.size() && e0 + i < fed.entries.size(); i++)
                CHECK(fed.entries[e0 + i].key == noted.entries[i].key && fed.entries[e0 + i].node == noted.entries[i].node);
        }
        AccmapIndex index;
        index.build(whole.entries);
        for (size_t i = 1; i < index.sorted.size(); i++) CHECK(!AccmapIndex::less(index.sorted[i].key, index.sorted[i - 1].key));
        for (size_t i = 0; i < whole.entries.size() && i < 2000; i++) {
            const std::string &key = whole.entries[i].key;
            int32_t first = -1;
            for (const auto &e : whole.entries)
                if (e.key == key) {
                    first = e.node;
                    break;
                }
            const std::string header = ">" + key + " some genome";
            std::vector<uint8_t> h(header.begin(), header.end());
            CHECK(index.lookup(h.data(), h.size(), false) == first);
            const bool complete = key.size() >= 3 && key[2] == '_' && key.compare(0, 2, "NG") != 0 && key.compare(0, 2, "NT") != 0 && key.compare(0, 2, "NW") != 0;
            CHECK(index.lookup(h.data(), h.size(), true) == (complete ? first : -1));
            std::vector<uint8_t> no_blank(header.begin(), header.begin() + 1 + (long)key.size());
            CHECK(index.lookup(no_blank.data(), no_blank.size(), false) == -1);
        }
    }
    fclose(f);
    printf("fails %d\n", fails);
    return fails != 0;
}
