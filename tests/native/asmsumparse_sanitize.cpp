// The record-by-record assembly summary parser of the host layer (genestrip_amd/csrc/gs_asmsumparse.h) on its own under
// AddressSanitizer / UBSan.  It reads the cases tests/test_asmsum_native_cpu.py writes out of tests/asmsum_cases.py (the hand-worked
// ones and generated text), prints what the parser and the cap make of each -- the test compares that with the expected values and
// with tests/asmsum.py -- and checks on its own that every split of a text into two feeds, at ANY byte (inside a line, between a CR
// and its LF), gives what one feed gives, and that a feed byte by byte does.
//
// The case file: n_cases, then per case the line `quality_mask reference_only use_species max_per_node`, `n_known` and one line of
// tax ids, `n_filter` and one line of flags (n_filter 0: no filter), `n_bytes`, and n_bytes of text followed by a newline.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../genestrip_amd/csrc/gs_asmsumparse.h"

using gs_host::AsmsumExact;

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

static bool feed(AsmsumExact &k, const std::string &s, bool last) {
    // (a copy of exactly the bytes, so that a read past either end is a heap overflow the sanitizer sees)
    std::vector<uint8_t> b(s.begin(), s.end());
    return k.feed(b.data(), b.size(), last);
}

static bool same(const AsmsumExact &a, const AsmsumExact &b) {
    if (a.counted != b.counted || a.short_records != b.short_records || a.skipped != b.skipped || a.line_no != b.line_no || a.entries.size() != b.entries.size())
        return false;
    for (size_t i = 0; i < a.entries.size(); i++) {
        const auto &x = a.entries[i], &y = b.entries[i];
        if (x.node != y.node || x.quality != y.quality || x.is_ref != y.is_ref || x.line != y.line || x.taxid != y.taxid || x.species != y.species || x.ftp != y.ftp)
            return false;
    }
    return true;
}

static void hex(const std::string &s) {
    printf(" ");
    if (s.empty()) printf("-");
    for (unsigned char b : s) printf("%02x", b);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int n_cases = atoi(read_line(f).c_str());
    for (int c = 0; c < n_cases; c++) {
        AsmsumExact proto;
        int mask = 0, ref = 0, species = 0, max_per_node = 0;
        sscanf(read_line(f).c_str(), "%d %d %d %d", &mask, &ref, &species, &max_per_node);
        proto.quality_mask = mask;
        proto.reference_only = ref != 0;
        proto.use_species = species != 0;
        for (int pass = 0; pass < 2; pass++) {
            const int n = atoi(read_line(f).c_str());
            const std::string vals = read_line(f);
            const char *p = vals.c_str();
            for (int i = 0; i < n; i++) {
                const long v = strtol(p, (char **)&p, 10);
                if (pass == 0)
                    proto.known.push_back((int32_t)v);
                else
                    proto.filter.push_back((uint8_t)v);
            }
        }
        const size_t n_bytes = (size_t)atoll(read_line(f).c_str());
        std::string text(n_bytes, '\0');
        CHECK(fread(&text[0], 1, n_bytes, f) == n_bytes);
        read_line(f);

        AsmsumExact whole = proto;
        if (!feed(whole, text, true)) {
            CHECK(!whole.error.empty());
            printf("case %d throws %lld\n", c, (long long)whole.line_no);
            AsmsumExact bytewise = proto;  // the same line, fed byte by byte
            bool ok = true;
            for (size_t i = 0; ok && i < text.size(); i++) ok = feed(bytewise, text.substr(i, 1), i + 1 == text.size());
            CHECK(!ok && bytewise.line_no == whole.line_no);
            continue;
        }
        gs_host::AsmsumStore store;
        store.entries = whole.entries;
        store.finish(max_per_node);
        printf("case %d ok %lld %lld %lld %lld %zu %zu %lld\n", c, (long long)whole.counted, (long long)whole.short_records, (long long)whole.skipped,
               (long long)whole.line_no, whole.entries.size(), store.picked.size(), (long long)store.nodes_with_entries);
        for (const auto &e : whole.entries) {
            printf("  e %d %d %d %lld", e.node, (int)e.quality, (int)e.is_ref, (long long)e.line);
            hex(e.taxid);
            hex(e.species);
            hex(e.ftp);
            printf("\n");
        }
        printf("  p");
        for (uint32_t i : store.picked) printf(" %u", i);
        printf("\n");
        // two feeds cut at any byte; at most 200 cuts of a long text, spread over it
        const size_t step = text.size() / 200 + 1;
        for (size_t cut = 0; cut <= text.size(); cut += (text.size() < 400 ? 1 : step)) {
            AsmsumExact k = proto;
            CHECK(feed(k, text.substr(0, cut), false) && feed(k, text.substr(cut), true));
            CHECK(same(k, whole));
        }
        if (text.size() < 20000) {
            AsmsumExact k = proto;
            bool ok = true;
            for (size_t i = 0; ok && i < text.size(); i++) ok = feed(k, text.substr(i, 1), false);
            CHECK(ok && feed(k, std::string(), true));
            CHECK(same(k, whole));
        }
    }
    fclose(f);
    printf("fails %d\n", fails);
    return fails != 0;
}
