// The line-by-line taxonomy parser and host tree of the library (genestrip_amd/csrc/gs_taxparse.h) on their own under
// AddressSanitizer / UBSan.  It reads the cases tests/test_taxtree_native_cpu.py writes out of tests/taxtree_cases.py (the hand-worked
// ones and generated dumps), prints what the parser and the tree make of each -- the test compares that with tests/taxtree.py -- and
// checks on its own that every split of a text into two feeds of whole lines gives what one feed gives, and that select and the small
// tree stay inside their arrays.
//
// The case file: n_cases, then per case `n_bytes` and that many bytes of nodes text followed by a newline, then the same for names.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "../../genestrip_amd/csrc/gs_taxparse.h"

using namespace gs_host;

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

static std::string read_block(FILE *f) {
    const size_t n = (size_t)atoll(read_line(f).c_str());
    std::string text(n, '\0');
    CHECK(fread(&text[0], 1, n, f) == n);
    read_line(f);
    return text;
}

// (a copy of exactly the bytes, so that a read past either end is a heap overflow the sanitizer sees)
static bool feed(TaxNodesExact &k, const std::string &s, bool last) {
    std::vector<uint8_t> b(s.begin(), s.end());
    return k.feed(b.data(), b.size(), last);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int n_cases = atoi(read_line(f).c_str());
    for (int c = 0; c < n_cases; c++) {
        const std::string nodes = read_block(f), names = read_block(f);
        auto whole = std::make_unique<TaxNodesExact>();
        if (!feed(*whole, nodes, true)) {
            CHECK(!whole->err.what.empty());
            printf("case %d fails %d %lld\n", c, whole->err.code, (long long)whole->err.line);
            continue;
        }
        size_t cuts = 0;
        for (size_t cut = 1; cut < nodes.size() && cuts < 48; cut++) {
            if (nodes[cut - 1] != '\n') continue;
            cuts++;
            auto k = std::make_unique<TaxNodesExact>();
            CHECK(feed(*k, nodes.substr(0, cut), false) && feed(*k, nodes.substr(cut), true));
            CHECK(k->line_no == whole->line_no && k->slots.size() == whole->slots.size());
            for (size_t i = 0; i < k->slots.size() && i < whole->slots.size(); i++)
                CHECK(k->slots[i].id == whole->slots[i].id && k->slots[i].parent == whole->slots[i].parent && k->slots[i].rank == whole->slots[i].rank);
        }
        TaxHostTree t;
        std::string why;
        std::vector<TaxSlot> slots(whole->slots);  // (exactly as many as there are)
        if (!t.build(slots.data(), slots.size(), &why)) {
            CHECK(!why.empty());
            printf("case %d fails 1 0\n", c);
            continue;
        }
        auto nm = std::make_unique<TaxNamesExact>();
        std::vector<uint8_t> nb(names.begin(), names.end());
        if (!nm->feed(t, nb.data(), nb.size(), true)) {
            printf("case %d names %d %lld\n", c, nm->err.code, (long long)nm->err.line);
            continue;
        }
        printf("case %d ok %d %lld %lld\n", c, t.n, (long long)t.duplicates, (long long)whole->line_no);
        for (int32_t v = 0; v < t.n; v++) {
            printf("  %d %d %d %d %d %d %d ", t.taxids[v], t.parent[v], t.depth[v], t.position[v], t.subtree[v], t.rank[v], (int)t.has_name[v]);
            for (unsigned char b : t.names[v]) printf("%02x", b);
            printf("\n");
        }
        // select and small over every node as the one request / flag (at most 64 of them): inside their arrays, and consistent
        for (int32_t v = 0; v < t.n && v < 64; v++) {
            std::vector<uint8_t> out((size_t)t.n), flags((size_t)t.n, 0);
            const bool ok = t.select(&v, 1, nullptr, 0, 21, out.data());
            if (ok) CHECK(out[(size_t)v] == 1);
            flags[(size_t)v] = 1;
            std::vector<int32_t> node_of_vi, parent_vi;
            t.small(flags.data(), node_of_vi, parent_vi);
            CHECK(node_of_vi.size() == parent_vi.size() && !node_of_vi.empty() && node_of_vi[0] == t.root && parent_vi[0] == -1);
            CHECK(t.position[(size_t)v] < 0 ? node_of_vi.size() == 1 : (int32_t)node_of_vi.size() >= t.depth[(size_t)v] + 1);
            for (size_t i = 1; i < node_of_vi.size(); i++) CHECK(parent_vi[i] >= 0 && parent_vi[i] < (int32_t)i);
        }
    }
    fclose(f);
    printf("fails %d\n", fails);
    return fails != 0;
}
