// accmap_emulate.cpp -- the kernels of genestrip_amd/csrc/gs_accmap.hip (tiles, count pass, write pass, the finish, the lookup)
// compiled for the host against a stand-in for the HIP constructs they use -- a block is 256 real threads, a wave 64 of them -- and
// run under AddressSanitizer / UBSan on generated chunks, every array exactly as large as gs_api.cpp makes it at the least (the text:
// its tiles and 64 zero bytes; per-tile arrays: tiles + 1; the entry arrays: the puts pass 1 counted).  What comes out is held to
// genestrip_amd/csrc/gs_accmapparse.h: counts, entries in input order, sorted order, duplicates, lookups.  Chunks of one line, of a
// tile less and more a byte, of several tiles; lines that end on every offset of a lane; fields across tile borders; an unterminated
// tail; refused chunks, which must name their first bad line.
// The test that builds it (tests/test_accmap_native_cpu.py) puts a <hip/hip_runtime.h> and a <rocprim/device/device_radix_sort.hpp>
// on the include path that both include accmap_emulate_hip.h (it holds a stable-sort stand-in for the one rocPRIM call).
#include "accmap_emulate_hip.h"
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
#include "../../genestrip_amd/csrc/gs_accmap.hip"
#include "../../genestrip_amd/csrc/gs_accmapparse.h"
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <string>

// n elements of T, 16-byte aligned, exactly: a byte more is a heap overflow the sanitizer sees
template <class T>
struct Exact {
    T *p;
    explicit Exact(size_t n) : p(nullptr) {
        if (posix_memalign((void **)&p, 16, (n ? n : 1) * sizeof(T))) abort();
        memset(p, 0, (n ? n : 1) * sizeof(T));
    }
    ~Exact() { free(p); }
};

static const std::vector<std::string> CATS = {"bacteria", "other"}, STATS = {"REVIEWED", "na"};
static const std::vector<int32_t> KNOWN = {7, 562, 9606, 10090};

static std::string line(std::mt19937_64 &rng, size_t name_len) {
    static const char *prefix[] = {"NC_", "NZ_", "NG_", "AC_", "WP_", "XP_", "NM_", "NC", "N"};
    static const char *cat[] = {"complete|bacteria", "vertebrate_other", "plant", "bacteri", "other"};
    static const char *stat[] = {"REVIEWED", "MODEL|national", "VALIDATED", "REVIEWE", "na"};
    static const char *tax[] = {"7", "562", "9606", "10090", "11", "999999999"};
    std::string acc = prefix[rng() % 9];
    for (size_t i = rng() % 20; i > 0; i--) acc += (char)('0' + rng() % 10);
    return std::string(tax[rng() % 6]) + "\t" + std::string(name_len, 'n') + "\t" + acc + "\t" + cat[rng() % 5] + "\t" + stat[rng() % 5] + "\t" +
           std::to_string(rng() % 100000) + "\n";
}

struct Result {
    bool refused = false;
    uint32_t bad_line = 0;
    u64 lines = 0, passing = 0, put = 0;
    std::vector<gs_host::AccmapEntry> entries;
};

// one chunk through both passes, as gs_accmap_submit drives them
static Result run_chunk(const std::string &text, bool last, const GsAccmapPatterns &pat, Exact<int32_t> &regions) {
    Result r;
    const int64_t n_bytes = (int64_t)text.size(), n_tiles = (n_bytes + GS_AM_TILE - 1) / GS_AM_TILE;
    Exact<uint8_t> d_text((size_t)n_tiles * GS_AM_TILE + 64);
    memcpy(d_text.p, text.data(), text.size());
    Exact<u64> tile_lt((size_t)n_tiles + 1), tile_put((size_t)n_tiles + 1), small(2 + GS_AM_C_WORDS);
    Exact<uint32_t> tile_tail((size_t)n_tiles + 1), status(GS_AM_WORDS);
    Exact<int32_t> known(KNOWN.size());
    memcpy(known.p, KNOWN.data(), KNOWN.size() * sizeof(int32_t));
    status.p[GS_AM_BAD_LINE] = GS_AM_NONE;
    GsAccmapParams P{};
    P.text = d_text.p; P.n_bytes = n_bytes; P.n_tiles = n_tiles; P.last = last; P.dna = 1; P.rna = 0; P.mrna = 0;
    P.n_cat = (int)CATS.size(); P.n_stat = (int)STATS.size(); P.pat = &pat; P.known = known.p; P.n_nodes = (int)KNOWN.size();
    P.tile_lt = tile_lt.p; P.tile_tail = tile_tail.p; P.tile_put = tile_put.p; P.scan_tot = small.p; P.status = status.p; P.chunk = small.p + 2;
    P.regions = regions.p;
    gs_launch_accmap_count(&P, nullptr);
    r.lines = P.chunk[GS_AM_C_LINES];
    if (status.p[GS_AM_BAD_LINE] != GS_AM_NONE) {
        r.refused = true;
        r.bad_line = status.p[GS_AM_BAD_LINE];
        return r;
    }
    r.passing = P.chunk[GS_AM_C_PASSING];
    r.put = P.chunk[GS_AM_C_PUT];
    Exact<uint8_t> keys((size_t)r.put * 32);
    Exact<int32_t> nodes((size_t)r.put);
    P.keys = keys.p; P.nodes = nodes.p; P.first_entry = 0; P.entry_cap = (int64_t)r.put;
    if (r.put) gs_launch_accmap_write(&P, nullptr);
    for (u64 i = 0; i < r.put; i++) r.entries.push_back({std::string((const char *)keys.p + 32 * i + 1, keys.p[32 * i]), nodes.p[i]});
    return r;
}

int main() {
    int fails = 0;
    GsAccmapPatterns pat{};
    gs_host::AccmapExact proto;
    proto.dna = true;
    proto.categories = CATS;
    proto.statuses = STATS;
    proto.known = KNOWN;
    for (size_t i = 0; i < CATS.size(); i++) { pat.len[i] = (uint8_t)CATS[i].size(); memcpy(pat.text[i], CATS[i].data(), CATS[i].size()); }
    for (size_t i = 0; i < STATS.size(); i++) { pat.len[GS_AM_MAX_PATTERNS + i] = (uint8_t)STATS[i].size(); memcpy(pat.text[GS_AM_MAX_PATTERNS + i], STATS[i].data(), STATS[i].size()); }
    Exact<int32_t> regions(KNOWN.size());
    std::vector<gs_host::AccmapEntry> all;
    std::vector<int32_t> want_regions(KNOWN.size(), 0);
    const size_t sizes[] = {1, 4095, 4096, 4097, 3 * 4096 + 100, 9 * 4096 + 5, 4096 + 2040};
    int seed = 0;
    for (size_t target : sizes) {
        for (int pad = 0; pad < 17; pad += target == 4096 ? 1 : target == 1 ? 17 : target < 4100 ? 4 : 8) {
            std::mt19937_64 rng(++seed);
            std::string text(pad, 'x');
            text += "\t\t\t\t\t\n";  // the pad line: the lines behind it start on every offset of a lane
            if (target == 1) text.clear();
            while (text.size() < target) {
                std::string ln = line(rng, rng() % 8 ? rng() % 30 : 150 + rng() % 1700);
                if (rng() % 40 == 0) ln = "\n";
                text += ln;
            }
            const bool last = seed % 3 == 0;
            if (last) text.pop_back();  // an unterminated tail
            gs_host::AccmapExact exact = proto;
            std::vector<uint8_t> copy(text.begin(), text.end());
            const bool parsed = exact.feed(copy.data(), copy.size(), last);
            const Result r = run_chunk(text, last, pat, regions);
            bool ok = parsed && !r.refused && r.lines == (u64)exact.lines && r.passing == (u64)exact.passing && r.entries.size() == exact.entries.size();
            for (size_t i = 0; ok && i < r.entries.size(); i++) ok = r.entries[i].key == exact.entries[i].key && r.entries[i].node == exact.entries[i].node;
            printf("seed %d bytes %zu pad %d last %d: lines %llu passing %llu put %llu (want %lld %lld %zu) %s\n", seed, text.size(), pad, (int)last, r.lines, r.passing,
                   r.put, (long long)exact.lines, (long long)exact.passing, exact.entries.size(), ok ? "ok" : "MISMATCH");
            fails += !ok;
            for (const auto &e : exact.entries) {
                all.push_back(e);
                want_regions[(size_t)e.node]++;
            }
        }
    }
    for (size_t i = 0; i < KNOWN.size(); i++) {
        if (regions.p[i] != want_regions[i]) { printf("regions of node %zu: %d, want %d MISMATCH\n", i, regions.p[i], want_regions[i]); fails++; }
    }
    {  // refusals name their first bad line
        std::mt19937_64 rng(99);
        std::string good;
        for (int i = 0; i < 90; i++) good += line(rng, 20);
        const struct { std::string bad; bool last; } cases[] = {
            {"7\tx\tNC_1\tbacteria\tREVIEWED\n", false}, {std::string("7\tx\tWP_1\ta") + '\0' + "\tb\tc\n", false}, {"07\tx\tNC_1\tbacteria\tREVIEWED\t1\n", false},
            {"7\tx\tNC_" + std::string(29, '1') + "\tbacteria\tREVIEWED\t1\n", false}, {"7\t" + std::string(2100, 'n') + "\tNC_1\tbacteria\tREVIEWED\t1\n", false},
            {"7\t" + std::string(9000, 'n') + "\tNC_1\tbacteria\tREVIEWED\t1\n", false}, {"7\tx\tNC_1\tbacteria\tREVIEWED\t1", false},
            {"7\t" + std::string(2030, 'n') + "\tNC_1\tbacteria\tREVIEWED\t1", true}};
        for (const auto &c : cases) {
            const std::string text = good + c.bad + (c.bad.back() == '\n' ? good : "");
            const Result r = run_chunk(text, c.last, pat, regions);
            const bool ok = r.refused && r.bad_line == 90;
            printf("refusal of %zu bytes: refused %d bad line %u (want 90) %s\n", text.size(), (int)r.refused, r.bad_line, ok ? "ok" : "MISMATCH");
            fails += !ok;
        }
    }
    // the finish and the lookup over everything that was put
    const int64_t n = (int64_t)all.size();
    Exact<uint8_t> keys((size_t)n * 32), keys_out((size_t)n * 32);
    Exact<int32_t> nodes((size_t)n), nodes_out((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        keys.p[32 * i] = (uint8_t)all[i].key.size();
        memcpy(keys.p + 32 * i + 1, all[i].key.data(), all[i].key.size());
        nodes.p[i] = all[i].node;
    }
    Exact<u64> word((size_t)n), word_alt((size_t)n), counts(2);
    Exact<uint32_t> seq((size_t)n), seq_alt((size_t)n), flag(1);
    size_t tmp_bytes = 0;
    gs_accmap_sort_bytes(n, &tmp_bytes);
    Exact<uint8_t> tmp(tmp_bytes);
    uint32_t *seq_sorted = nullptr;
    gs_accmap_sort_entries(keys.p, nodes.p, n, word.p, word_alt.p, seq.p, seq_alt.p, tmp.p, tmp_bytes, flag.p, keys_out.p, nodes_out.p, &seq_sorted, counts.p, nullptr);
    gs_host::AccmapIndex index;
    index.build(all);
    u64 dup = 0, conflicts = 0;
    bool ok = true;
    for (int64_t i = 0; i < n; i++) {
        ok = ok && std::string((const char *)keys_out.p + 32 * i + 1, keys_out.p[32 * i]) == index.sorted[i].key && nodes_out.p[i] == index.sorted[i].node;
        if (i && index.sorted[i].key == index.sorted[i - 1].key) { dup++; conflicts += index.sorted[i].node != index.sorted[i - 1].node; }
    }
    ok = ok && counts.p[0] == dup && counts.p[1] == conflicts && n > 100 && dup > 0;
    printf("finish of %lld entries: duplicates %llu (want %llu) conflicts %llu (want %llu) %s\n", (long long)n, counts.p[0], dup, counts.p[1], conflicts, ok ? "ok" : "MISMATCH");
    fails += !ok;
    for (int complete = 0; complete < 2; complete++) {
        std::mt19937_64 rng(7);
        std::vector<std::string> hs = {">", "", "> x", ">" + std::string(32, 'N') + " x", ">NC_1", " >NC_1 x"};
        for (int i = 0; i < 500; i++) {
            std::string k = all[rng() % all.size()].key;
            if (i % 5 == 0) k += "9";
            hs.push_back(">" + k + (i % 7 ? " some genome" : ""));
        }
        std::vector<u64> off{0};
        std::string flat;
        for (const auto &h : hs) { flat += h; off.push_back(flat.size()); }
        Exact<uint8_t> d_h(flat.size());
        memcpy(d_h.p, flat.data(), flat.size());
        Exact<u64> d_off(off.size());
        memcpy(d_off.p, off.data(), off.size() * sizeof(u64));
        Exact<int32_t> out(hs.size());
        gs_launch_accmap_lookup(d_h.p, d_off.p, (int64_t)hs.size(), complete, keys_out.p, nodes_out.p, n, out.p, nullptr);
        bool same = true;
        int found = 0;
        for (size_t i = 0; i < hs.size(); i++) {
            std::vector<uint8_t> h(hs[i].begin(), hs[i].end());
            same = same && out.p[i] == index.lookup(h.data(), h.size(), complete != 0);
            found += out.p[i] >= 0;
        }
        printf("lookup of %zu headers, complete_only %d: %d found %s\n", hs.size(), complete, found, same && found > 100 ? "ok" : "MISMATCH");
        fails += !(same && found > 100);
    }
    printf("fails %d\n", fails);
    return fails != 0;
}
