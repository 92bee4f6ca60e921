// taxtree_emulate.cpp -- the kernels of genestrip_amd/csrc/gs_taxtree.hip (tiles, nodes scan, the three names passes, the finish,
// select, small tree) compiled for the host against a stand-in for the HIP constructs they use -- a block is 256 real threads, a
// wave 64 of them -- and run under AddressSanitizer / UBSan, every array exactly as large as gs_api.cpp makes it at the least (the
// text: its tiles and 64 zero bytes; per-tile arrays: tiles + 1; slots: the lines; the finish scratch: 8m and 22n + 16 words; select:
// 2n bytes and 3n words and the lists; small tree: 8 words per reached node and the flags; the pool: what is used and the chunk).
// What comes out is held to genestrip_amd/csrc/gs_taxparse.h.  The test that builds it (tests/test_taxtree_native_cpu.py) puts a
// <hip/hip_runtime.h> and the two rocPRIM headers on the include path that all include taxtree_emulate_hip.h.
#include "taxtree_emulate_hip.h"
thread_local dim3 threadIdx, blockIdx;
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
#include "../../genestrip_amd/csrc/gs_taxtree.hip"
#include "../../genestrip_amd/csrc/gs_taxparse.h"
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <string>

using namespace gs_host;

template <class T>
struct Exact {  // n elements of T, 16-byte aligned, exactly: a byte more is a heap overflow the sanitizer sees
    T *p;
    explicit Exact(size_t n) : p(nullptr) {
        if (posix_memalign((void **)&p, 16, (n ? n : 1) * sizeof(T))) abort();
        memset(p, 0, (n ? n : 1) * sizeof(T));
    }
    ~Exact() { free(p); }
};

static int fails = 0;
#define CHECK(c)                                            \
    do {                                                    \
        if (!(c)) {                                         \
            fails++;                                        \
            printf("MISMATCH line %d: %s\n", __LINE__, #c); \
        }                                                   \
    } while (0)

static GsTaxRanks g_ranks;

struct Chunk {
    Exact<uint8_t> text;
    Exact<u64> tile_lb, small;
    Exact<uint32_t> tile_tail;
    GsTaxScanParams P{};
    int64_t n_lines = 0;
    Chunk(const std::string &s, bool last)
        : text(((s.size() + GS_TT_TILE - 1) / GS_TT_TILE) * GS_TT_TILE + 64), tile_lb((s.size() + GS_TT_TILE - 1) / GS_TT_TILE + 1), small(2),
          tile_tail((s.size() + GS_TT_TILE - 1) / GS_TT_TILE + 1) {
        memcpy(text.p, s.data(), s.size());
        small.p[0] = (u64)GS_TT_NONE;
        P.text = text.p; P.n_bytes = (int64_t)s.size(); P.n_tiles = (P.n_bytes + GS_TT_TILE - 1) / GS_TT_TILE; P.last = last; P.ranks = &g_ranks;
        P.tile_lb = tile_lb.p; P.tile_tail = tile_tail.p; P.scan_tot = small.p + 1; P.status = (uint32_t *)small.p;
        gs_launch_taxtree_tiles(&P, nullptr);
        n_lines = (int64_t)(uint32_t)small.p[1] + (s.back() != '\n');
    }
    uint32_t bad() const { return (uint32_t)small.p[0]; }
};

// a chunk of nodes lines as gs_taxtree_submit_nodes drives it; false: refused (then *bad_line says where)
static bool scan_nodes(const std::string &s, bool last, std::vector<TaxSlot> &slots, uint32_t *bad_line) {
    Chunk c(s, last);
    Exact<uint4> d_slots(slots.size() + (size_t)c.n_lines);
    if (!slots.empty()) memcpy(d_slots.p, slots.data(), slots.size() * sizeof(uint4));
    c.P.slots = d_slots.p; c.P.first_line = (int64_t)slots.size(); c.P.slot_cap = (int64_t)slots.size() + c.n_lines;
    gs_launch_taxtree_scan(&c.P, nullptr);
    *bad_line = c.bad();
    if (c.bad() != GS_TT_NONE) return false;
    slots.resize(slots.size() + (size_t)c.n_lines);
    memcpy(slots.data(), d_slots.p, slots.size() * sizeof(uint4));
    return true;
}

struct DeviceTree {
    int32_t n = 0, n_reach = 0;
    u64 dups = 0;
    std::vector<int32_t> taxids, parent, rank, depth, position, subtree, node_at, line_of;
    std::vector<uint8_t> cyc;
    GsTaxTreeArrays A{};
};

// gs_taxtree_finish_nodes, step by step with its sizes; false: no root or duplicates
static bool finish(const std::vector<TaxSlot> &slots, DeviceTree &t) {
    const int64_t m = (int64_t)slots.size();
    Exact<uint4> d_slots((size_t)m);
    memcpy(d_slots.p, slots.data(), (size_t)m * sizeof(uint4));
    Exact<u64> counts(6);
    size_t tmp_bytes = 0;
    gs_taxtree_sort_bytes(2 * m, &tmp_bytes);
    Exact<uint8_t> tmp(tmp_bytes);
    t.taxids.assign((size_t)(2 * m), 0);
    {
        Exact<uint32_t> w((size_t)(8 * m));
        Exact<int32_t> taxids((size_t)(2 * m));
        gs_taxtree_distinct(d_slots.p, m, w.p, w.p + 2 * m, w.p + 4 * m, w.p + 6 * m, tmp.p, tmp_bytes, taxids.p, counts.p, nullptr);
        memcpy(t.taxids.data(), taxids.p, (size_t)(2 * m) * sizeof(int32_t));
    }
    t.n = (int32_t)((uint32_t)counts.p[4] + (uint32_t)(counts.p[4] >> 32));
    if (t.n <= 0) return false;
    const size_t N = (size_t)t.n;
    t.taxids.resize(N);
    for (auto *v : {&t.parent, &t.rank, &t.depth, &t.position, &t.subtree, &t.node_at, &t.line_of}) v->assign(N, 0);
    t.cyc.assign(N, 0);
    t.A.n = t.n; t.A.root = 0; t.A.taxids = t.taxids.data(); t.A.parent = t.parent.data(); t.A.rank = t.rank.data(); t.A.line_of = t.line_of.data();
    t.A.depth = t.depth.data(); t.A.position = t.position.data(); t.A.subtree = t.subtree.data(); t.A.node_at = t.node_at.data(); t.A.cyc = t.cyc.data();
    gs_taxtree_resolve(d_slots.p, m, &t.A, counts.p, nullptr);
    t.dups = counts.p[0];
    if (t.dups || t.taxids[0] != 1 || t.parent[0] != -1 || t.line_of[0] < 0) return false;
    Exact<uint32_t> w(22 * N + 16);
    u64 *key = (u64 *)w.p;
    uint32_t *ord = w.p + 4 * N, *succ = w.p + 8 * N;
    int32_t *first_child = (int32_t *)(w.p + 6 * N), *next_sib = (int32_t *)(w.p + 7 * N);
    u64 *val = (u64 *)(w.p + 8 * N + 2 * (2 * N + 2));
    int32_t *up = (int32_t *)(w.p + 8 * N + 2 * (2 * N + 2) + 4 * (2 * N + 2));
    gs_taxtree_children(&t.A, key, key + N, ord, ord + N, tmp.p, tmp_bytes, first_child, next_sib, nullptr);
    gs_taxtree_place(&t.A, first_child, next_sib, succ, succ + 2 * N + 2, val, val + 2 * N + 2, up, up + N, counts.p, nullptr);
    t.n_reach = (int32_t)counts.p[1];
    return true;
}

static std::string node_line(int id, int parent, const char *rank, size_t pad) {
    return std::to_string(id) + "\t|\t" + std::to_string(parent) + "\t|\t" + rank + "\t|\t" + std::string(pad, 'x') + "\t|\n";
}

int main() {
    for (int r = 0; r < GS_TT_N_RANKS; r++) {
        g_ranks.len[r] = (uint8_t)strlen(TAX_RANK_NAMES[r]);
        memcpy(g_ranks.text[r], TAX_RANK_NAMES[r], g_ranks.len[r]);
    }
    static const char *ranks[] = {"no rank", "species", "genus", "strain", "clade", "forma specialis", "odd", "", "superkingdom"};
    std::mt19937_64 rng(7);
    int oks = 0;
    for (int round = 0; round < 3; round++) {
        // a tree of some hundred nodes in shuffled line order, with a parent-only node, a second root and a two-cycle with a tail;
        // round 1: a chain; pads move lines over tile and lane borders, one line is 4096 bytes
        const int n = round == 1 ? 500 : 300 + 150 * round;
        std::vector<std::string> lines;
        lines.push_back(node_line(1, 1, "no rank", 0));
        for (int i = 2; i <= n; i++)
        {
            const int parent = i == 2 ? 1 : round == 1 ? (i - 1) * 3 : (rng() % 8 == 0 ? 1 : (int)(2 + rng() % (i - 2)) * 3);
            lines.push_back(node_line(i * 3, parent, ranks[rng() % 9], rng() % 40));
        }
        if (round != 1) {
            lines.push_back(node_line(5000, 7777, "species", 0));   // a parent no line introduces
            lines.push_back(node_line(6001, 6001, "no rank", 3));   // a second self-parent node with a child
            lines.push_back(node_line(6002, 6001, "species", 0));
            lines.push_back(node_line(8000, 8002, "genus", 0));     // a two-cycle with a tail
            lines.push_back(node_line(8002, 8000, "genus", 0));
            lines.push_back(node_line(8004, 8002, "species", 0));
            std::string big = node_line(9001, 1, "species", 0);
            big.insert(big.size() - 3, std::string(4096 - big.size(), 'y'));
            lines.push_back(big);
            lines.push_back("\n");
            std::shuffle(lines.begin(), lines.end(), rng);
        }
        std::string text;
        for (auto &l : lines) text += l;
        if (round == 2) text.pop_back();  // an unterminated tail
        // the host's answer
        TaxNodesExact exact;
        CHECK(exact.feed((const uint8_t *)text.data(), text.size(), true));
        TaxHostTree want;
        std::string why;
        CHECK(want.build(exact.slots.data(), exact.slots.size(), &why));
        // the device's: as one chunk, and cut behind a line near every tile border
        for (int cut_mode = 0; cut_mode < 2; cut_mode++) {
            std::vector<TaxSlot> slots;
            uint32_t bad = 0;
            size_t from = 0;
            while (from < text.size()) {
                size_t to = text.size();
                if (cut_mode) {
                    const size_t aim = std::min(text.size(), from + 4096 + rng() % 64);
                    const size_t nl = text.find('\n', aim > 0 ? aim - 1 : 0);
                    to = nl == std::string::npos ? text.size() : nl + 1;
                }
                CHECK(scan_nodes(text.substr(from, to - from), to == text.size(), slots, &bad));
                from = to;
            }
            DeviceTree t;
            CHECK(finish(slots, t));
            CHECK(t.n == want.n && t.taxids == want.taxids && t.parent == want.parent && t.rank == want.rank);
            CHECK(t.depth == want.depth && t.position == want.position && t.subtree == want.subtree);
            for (int32_t v = 0; v < t.n; v++) CHECK(t.cyc[(size_t)v] == (round != 1 && (t.taxids[(size_t)v] == 8000 || t.taxids[(size_t)v] == 8002)));
            if (cut_mode) continue;
            const size_t N = (size_t)t.n;
            // select: random requests, excludes and cuts
            for (int turn = 0; turn < 3; turn++) {
                std::vector<int32_t> req, exc;
                for (int i = 0; i < 6; i++) {
                    int32_t v = (int32_t)(rng() % N);
                    if (!t.cyc[(size_t)v]) (i < 4 ? req : exc).push_back(v);
                }
                const int cut = turn == 0 ? -1 : turn == 1 ? 21 : 18;
                Exact<uint8_t> bytes(2 * N);
                Exact<int32_t> words(3 * N + req.size() + exc.size() + 1);
                memcpy(words.p + 3 * N, req.data(), req.size() * sizeof(int32_t));
                memcpy(words.p + 3 * N + req.size(), exc.data(), exc.size() * sizeof(int32_t));
                u64 count = 0;
                gs_launch_taxtree_select(&t.A, words.p + 3 * N, (int64_t)req.size(), words.p + 3 * N + req.size(), (int64_t)exc.size(), cut, bytes.p, words.p,
                                         bytes.p + N, &count, nullptr);
                std::vector<uint8_t> out(N);
                CHECK(want.select(req.data(), (int64_t)req.size(), exc.data(), (int64_t)exc.size(), cut, out.data()));
                CHECK(memcmp(out.data(), bytes.p + N, N) == 0);
                u64 sum = 0;
                for (uint8_t b : out) sum += b;
                CHECK(sum == count);
            }
            // small tree: flags as bytes and as counts
            for (int turn = 0; turn < 2; turn++) {
                const size_t R = (size_t)t.n_reach;
                std::vector<uint8_t> f8(N);
                std::vector<int32_t> f32(N);
                for (size_t v = 0; v < N; v++) {
                    f8[v] = rng() % 20 == 0;
                    f32[v] = f8[v] ? 1 + (int32_t)(rng() % 5) : -(int32_t)(rng() % 2);
                }
                const size_t flag_words = turn ? N : (N + 3) / 4;
                Exact<uint32_t> w(8 * R + flag_words + 1);
                memcpy(w.p + 8 * R, turn ? (const void *)f32.data() : (const void *)f8.data(), turn ? N * 4 : N);
                size_t tmp_bytes = 0;
                gs_taxtree_sort_bytes((int64_t)R, &tmp_bytes);
                Exact<uint8_t> tmp(tmp_bytes);
                gs_launch_taxtree_small(&t.A, t.n_reach, turn ? nullptr : (const uint8_t *)(w.p + 8 * R), turn ? (const int32_t *)(w.p + 8 * R) : nullptr, w.p, w.p + R,
                                        w.p + 2 * R, w.p + 3 * R, tmp.p, tmp_bytes, (int32_t *)(w.p + 4 * R), (int32_t *)(w.p + 5 * R), (int32_t *)(w.p + 6 * R),
                                        (int32_t *)(w.p + 7 * R), nullptr);
                const size_t S = (size_t)w.p[3 * R - 1] + w.p[4 * R - 1];
                std::vector<int32_t> nodes, parents;
                want.small(f8.data(), nodes, parents);
                CHECK(S == nodes.size());
                for (size_t i = 0; i < S && i < nodes.size(); i++)
                    CHECK((int32_t)w.p[4 * R + i] == nodes[i] && (int32_t)w.p[5 * R + i] == parents[i] && (int32_t)w.p[6 * R + i] == want.depth[(size_t)nodes[i]] &&
                          (int32_t)w.p[7 * R + i] == want.position[(size_t)nodes[i]]);
            }
            // names: synonyms and scientific lines in shuffled order, unknown and odd ids; chunks by turns on the device and refused
            std::vector<std::string> nl;
            for (size_t v = 0; v < N; v += 1 + rng() % 2) {
                const std::string id = std::to_string(t.taxids[v]);
                for (int k = (int)(rng() % 3); k > 0; k--) nl.push_back(id + "\t|\tsyn " + std::to_string(rng() % 1000) + "\t|\t\t|\tsynonym\t|\n");
                for (int k = (int)(rng() % 3); k > 0; k--) nl.push_back(id + "\t|\tSci " + std::to_string(rng() % 1000) + std::string(rng() % 30, 'z') + "\t|\t\t|\tscientific name\t|\n");
            }
            nl.push_back("4\t|\tnobody\t|\t\t|\tsynonym\t|\n");
            nl.push_back("0x\t|\tnobody\t|\t\t|\tscientific name\t|\n");
            nl.push_back("\n");
            std::shuffle(nl.begin(), nl.end(), rng);
            std::string names;
            for (auto &l : nl) names += l;
            TaxNamesExact nx;
            CHECK(nx.feed(want, (const uint8_t *)names.data(), names.size(), true));
            Exact<u64> win(N), name_off(N), pool_used(1);
            Exact<uint32_t> name_len(N);
            int64_t line_no = 0;
            std::vector<uint8_t> pool_now;
            for (size_t from = 0; from < names.size();) {
                const size_t aim = std::min(names.size(), from + 3000 + rng() % 3000);
                const size_t e = names.find('\n', aim > 0 ? aim - 1 : 0);
                const size_t to = e == std::string::npos ? names.size() : e + 1;
                Chunk c(names.substr(from, to - from), to == names.size());
                c.P.first_line = line_no; c.P.taxids = t.taxids.data(); c.P.n_nodes = t.n; c.P.win = win.p; c.P.name_off = name_off.p; c.P.name_len = name_len.p;
                c.P.pool_used = pool_used.p;
                gs_launch_taxtree_names(&c.P, 0, nullptr);
                CHECK(c.bad() == GS_TT_NONE);
                Exact<uint8_t> pool((size_t)pool_used.p[0] + (to - from));  // what is used and every name of the chunk
                if (!pool_now.empty()) memcpy(pool.p, pool_now.data(), pool_now.size());
                c.P.pool = pool.p;
                gs_launch_taxtree_names(&c.P, 1, nullptr);
                gs_launch_taxtree_names(&c.P, 2, nullptr);
                pool_now.assign(pool.p, pool.p + pool_used.p[0]);
                line_no += c.n_lines;
                from = to;
            }
            for (size_t v = 0; v < N; v++) {
                CHECK((win.p[v] != 0) == (want.has_name[v] != 0) && win.p[v] == want.name_key[v]);
                if (win.p[v]) CHECK(name_off.p[v] + name_len.p[v] <= pool_now.size() && std::string((const char *)pool_now.data() + name_off.p[v], name_len.p[v]) == want.names[v]);
            }
            // a line of a known node with a name of negative length refuses its chunk, and names its line
            Chunk bad_chunk("1\t|\tok\t|\n1\t||\n", true);
            bad_chunk.P.taxids = t.taxids.data(); bad_chunk.P.n_nodes = t.n;
            gs_launch_taxtree_names(&bad_chunk.P, 0, nullptr);
            CHECK(bad_chunk.bad() == 1);
        }
        // refusals of the nodes scan name their first bad line
        {
            std::vector<TaxSlot> slots;
            uint32_t bad = 0;
            CHECK(!scan_nodes(lines[0] + lines[1] + "02\t|\t1\t|\tspecies\t|\n" + lines[2], true, slots, &bad) && bad == 2 && slots.empty());
            CHECK(!scan_nodes(lines[0] + "7\t|\t1\t|\n", true, slots, &bad) && bad == 1);
            CHECK(!scan_nodes(lines[0] + "7\t|\t1\t|\tspecies\t|", false, slots, &bad) && bad == 1);
        }
        if (!fails) oks++;
        printf("round %d %s\n", round, fails ? "MISMATCH" : "ok");
    }
    printf("fails %d\n", fails);
    return fails != 0;
}
