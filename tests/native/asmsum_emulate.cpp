// asmsum_emulate.cpp -- the kernels of genestrip_amd/csrc/gs_asmsum.hip (tiles, slots, judge, write, gather, the cap, the picks)
// compiled for the host against a stand-in for the HIP constructs they use -- a block is 256 real threads, a wave 64 of them -- and
// run under AddressSanitizer / UBSan on generated chunks, every array exactly as large as gs_api.cpp makes it at the least (the text:
// its tiles and 64 zero bytes; per-tile arrays: tiles + 1; per-line arrays: the lines; per-block: blocks + 1; entries and pool: what
// the judge pass counted).  What comes out is held to genestrip_amd/csrc/gs_asmsumparse.h: counts, entries in input order with
// their strings and lines, refusals with their first bad line, the cap.  Chunks of one byte, of a tile less and more a byte, of
// several tiles; lines that start on every offset of a lane; an unterminated tail.
// The test that builds it (tests/test_asmsum_native_cpu.py) puts a <hip/hip_runtime.h> and the two rocPRIM headers on the include
// path that all include asmsum_emulate_hip.h.
#include "asmsum_emulate_hip.h"
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
#include "../../genestrip_amd/csrc/gs_asmsum.hip"
#include "../../genestrip_amd/csrc/gs_asmsumparse.h"
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <string>

// n elements of T, 32-byte aligned, exactly: a byte more is a heap overflow the sanitizer sees
template <class T>
struct Exact {
    T *p;
    explicit Exact(size_t n) : p(nullptr) {
        if (posix_memalign((void **)&p, 32, (n ? n : 1) * sizeof(T))) abort();
        memset(p, 0xa5, (n ? n : 1) * sizeof(T));  // (nothing relies on zeroed memory but what the library zeroes)
    }
    ~Exact() { free(p); }
};

static const std::vector<int32_t> KNOWN = {7, 562, 9606, 10090, 999999999};
static const std::vector<uint8_t> FILTER = {1, 1, 0, 1, 1};

static std::string line(std::mt19937_64 &rng, size_t name_len) {
    static const char *cat[] = {"reference genome", "representative genome", "na", "reference genom"};
    static const char *tax[] = {"7", "562", "9606", "10090", "11", "999999999", "007", "", "56x", "1234567890"};
    static const char *status[] = {"latest", "latest", "replaced", "Latest", "latest "};
    static const char *level[] = {"Complete Genome", "Chromosome", "Scaffold", "Contig", "complete genome", ""};
    static const char *ftp[] = {"https://ftp.ncbi.nlm.nih.gov/genomes/all/GCA/000/001/405/GCA_000001405.29_GRCh38.p14", "na", "/", "a/b/", "x"};
    const unsigned r = (unsigned)(rng() % 50);
    if (r == 0) return "\n";
    if (r == 1) return "#comment\twith\ttabs\n";
    std::string f[24];
    const int n_fields = r == 2 ? 1 + (int)(rng() % 19) : r == 3 ? 20 : 21 + (int)(rng() % 3);
    for (int i = 0; i < n_fields; i++) f[i] = "f" + std::to_string(rng() % 1000);
    f[4] = cat[rng() % 4];
    f[5] = tax[rng() % 10];
    f[6] = tax[rng() % 10];
    f[7] = std::string(name_len, 'n') + "\xc3\xbc";  // (a byte from 0x80 on outside the key fields is data)
    f[10] = status[rng() % 5];
    f[11] = level[rng() % 6];
    f[19] = ftp[rng() % 5];
    std::string out;
    for (int i = 0; i < n_fields; i++) out += (i ? "\t" : "") + f[i];
    if (r == 4) out += "\t";
    return out + "\n";
}

struct Result {
    bool refused = false;
    uint32_t bad_line = 0;
    u64 counted = 0, kept = 0, short_records = 0, skipped = 0, pool = 0;
    int64_t n_lines = 0;
    std::vector<gs_host::AsmsumEntry> entries;
};

struct Cfg {
    int key_field = 5, quality_mask = -1, reference_only = 0;
    bool filter = false;
};

// one chunk through the passes, as gs_asmsum_submit drives them
static Result run_chunk(const std::string &text, bool last, const Cfg &cfg, int64_t first_line) {
    Result r;
    const int64_t n_bytes = (int64_t)text.size(), n_tiles = (n_bytes + GS_AS_TILE - 1) / GS_AS_TILE;
    Exact<uint8_t> d_text((size_t)n_tiles * GS_AS_TILE + 64);
    memset(d_text.p, 0, (size_t)n_tiles * GS_AS_TILE + 64);
    memcpy(d_text.p, text.data(), text.size());
    Exact<u64> tile_lt((size_t)n_tiles + 1), small(2 + GS_AS_C_WORDS);
    Exact<uint32_t> tile_tail((size_t)n_tiles + 1), status(GS_AS_WORDS);
    Exact<int32_t> known(KNOWN.size());
    Exact<uint8_t> filter(FILTER.size());
    memcpy(known.p, KNOWN.data(), KNOWN.size() * sizeof(int32_t));
    memcpy(filter.p, FILTER.data(), FILTER.size());
    memset(small.p, 0, (2 + GS_AS_C_WORDS) * sizeof(u64));
    status.p[GS_AS_BAD_LINE] = GS_AS_NONE;
    status.p[GS_AS_LONGEST] = 0;
    GsAsmsumParams P{};
    P.text = d_text.p; P.n_bytes = n_bytes; P.n_tiles = n_tiles; P.last = last; P.key_field = cfg.key_field; P.quality_mask = cfg.quality_mask;
    P.reference_only = cfg.reference_only; P.known = known.p; P.filter = cfg.filter ? filter.p : nullptr; P.n_nodes = (int)KNOWN.size();
    P.tile_lt = tile_lt.p; P.tile_tail = tile_tail.p; P.scan_tot = small.p; P.status = status.p; P.chunk = small.p + 2;
    gs_launch_asmsum_tiles(&P, nullptr);
    const int64_t n_lines = (int64_t)(small.p[0] & 0xffffffffull) + (text.back() != '\n');
    const int64_t n_blocks = (n_lines + GS_AS_LINE_BLOCK - 1) / GS_AS_LINE_BLOCK;
    Exact<uint16_t> slots((size_t)n_lines * GS_AS_SLOT);
    Exact<uint8_t> high((size_t)n_lines);
    Exact<u64> verdict((size_t)n_lines), line_blk((size_t)n_blocks + 1);
    memset(high.p, 0, (size_t)n_lines);
    P.n_lines = n_lines; P.slots = slots.p; P.high = high.p; P.verdict = verdict.p; P.line_blk = line_blk.p;
    gs_launch_asmsum_judge(&P, nullptr);
    r.n_lines = n_lines;
    if (status.p[GS_AS_BAD_LINE] != GS_AS_NONE) {
        r.refused = true;
        r.bad_line = status.p[GS_AS_BAD_LINE];
        return r;
    }
    r.counted = P.chunk[GS_AS_C_COUNTED];
    r.kept = P.chunk[GS_AS_C_KEPT];
    r.short_records = P.chunk[GS_AS_C_SHORT];
    r.skipped = P.chunk[GS_AS_C_SKIPPED];
    r.pool = P.chunk[GS_AS_C_POOL];
    Exact<GsAsmEntry> entries((size_t)r.kept);
    Exact<uint8_t> pool((size_t)r.pool);
    Exact<uint32_t> put_line((size_t)r.kept);
    P.entries = entries.p; P.first_entry = 0; P.entry_cap = (int64_t)r.kept; P.first_line = first_line; P.pool = pool.p; P.pool_used = 0; P.pool_cap = r.pool;
    P.put_line = put_line.p;
    gs_launch_asmsum_write(&P, (int64_t)r.kept, nullptr);
    for (u64 i = 0; i < r.kept; i++) {
        const GsAsmEntry &e = entries.p[i];
        gs_host::AsmsumEntry h;
        h.node = e.node;
        h.quality = (uint8_t)(e.meta & 0xff);
        h.is_ref = (uint8_t)(e.meta >> 8 & 1);
        h.line = e.line;
        const char *s = (const char *)pool.p + e.pool_off;
        h.taxid.assign(s, e.len[0]);
        h.species.assign(s + e.len[0], e.len[1]);
        h.ftp.assign(s + e.len[0] + e.len[1], e.len[2]);
        r.entries.push_back(h);
    }
    return r;
}

static bool same(const gs_host::AsmsumEntry &a, const gs_host::AsmsumEntry &b) {
    return a.node == b.node && a.quality == b.quality && a.is_ref == b.is_ref && a.line == b.line && a.taxid == b.taxid && a.species == b.species && a.ftp == b.ftp;
}

static gs_host::AsmsumExact exact_of(const Cfg &cfg) {
    gs_host::AsmsumExact x;
    x.known = KNOWN;
    if (cfg.filter) x.filter = FILTER;
    x.quality_mask = cfg.quality_mask;
    x.reference_only = cfg.reference_only != 0;
    x.use_species = cfg.key_field == 6;
    return x;
}

int main() {
    int fails = 0;
    std::vector<gs_host::AsmsumEntry> all;
    const size_t sizes[] = {1, 4095, 4096, 4097, 3 * 4096 + 100, 9 * 4096 + 5, 4096 + 2040};
    int seed = 0;
    for (size_t target : sizes) {
        for (int pad = 0; pad < 17; pad += target == 4096 ? 1 : target == 1 ? 17 : target < 4100 ? 4 : 8) {
            std::mt19937_64 rng(++seed);
            Cfg cfg;
            cfg.key_field = seed % 2 ? 5 : 6;
            cfg.quality_mask = seed % 3 == 0 ? -1 : seed % 3 == 1 ? (1 << 1 | 1 << 3) : 0x7fe & ~(1 << 10);
            cfg.reference_only = seed % 5 == 0;
            cfg.filter = seed % 4 == 1;
            std::string text(pad, 'x');
            text += "\n";  // the pad line: the lines behind it start on every offset of a lane
            if (target == 1) text = "x";
            while (text.size() < target) {
                std::string ln = line(rng, rng() % 8 ? rng() % 30 : 150 + rng() % 3000);
                // (the generator's empty ftp path "" does not occur; an entry with "/" is kept with an empty base)
                text += ln;
            }
            const bool last = seed % 3 == 0 || target == 1;
            if (last && text.size() > 1) text.pop_back();  // an unterminated tail
            gs_host::AsmsumExact exact = exact_of(cfg);
            std::vector<uint8_t> copy(text.begin(), text.end());
            const bool parsed = exact.feed(copy.data(), copy.size(), last);
            const Result r = run_chunk(text, last, cfg, 1000);
            bool ok = parsed && !r.refused && r.counted == (u64)exact.counted && r.short_records == (u64)exact.short_records &&
                      r.skipped == (u64)exact.skipped && r.n_lines == exact.line_no && r.entries.size() == exact.entries.size();
            for (size_t i = 0; ok && i < r.entries.size(); i++) {
                gs_host::AsmsumEntry want = exact.entries[i];
                want.line += 1000;
                ok = same(r.entries[i], want);
            }
            printf("seed %d bytes %zu pad %d last %d: counted %llu kept %llu short %llu skipped %llu (want %lld %zu %lld %lld) %s\n", seed, text.size(), pad,
                   (int)last, r.counted, r.kept, r.short_records, r.skipped, (long long)exact.counted, exact.entries.size(), (long long)exact.short_records,
                   (long long)exact.skipped, ok ? "ok" : "MISMATCH");
            fails += !ok;
            for (const auto &e : exact.entries) all.push_back(e);
        }
    }
    {  // refusals name their first bad line
        std::mt19937_64 rng(99);
        std::string good;
        for (int i = 0; i < 90; i++) good += line(rng, 20);
        const std::string head = "a\tb\tc\td\treference genome\t", mid = "\t562\tn\ti\tj\tlatest\tComplete Genome\tm\tn\to\tp\tq\tr\ts\t";
        const struct { std::string bad; bool last; } cases[] = {
            {head + "7" + mid + "ftp\r\n", false},                                   // CR
            {"short\rline\n", false},                                                // CR in a short record
            {head + "\xc4\xb1" + mid + "ftp\n", false},                              // a byte from 0x80 on in the key field
            {head + "7" + mid + "\n", false},                                        // a kept entry with an empty ftp path
            {head + "7" + mid + "\textra\n", false},                                 // the same, a field behind it
            {head + "7" + mid + std::string(4096, 'f') + "\n", false},               // above the limit
            {head + "7" + mid + std::string(9000, 'f') + "\n", false},               // a line that covers two tiles
            {head + "7" + mid + "ftp", false},                                       // an unterminated tail inside the stream
        };
        for (const auto &c : cases) {
            const std::string text = good + c.bad + (c.bad.back() == '\n' ? good : "");
            const Result r = run_chunk(text, c.last, Cfg(), 0);
            const bool ok = r.refused && r.bad_line == 90;
            printf("refusal of %zu bytes: refused %d bad line %u (want 90) %s\n", text.size(), (int)r.refused, r.bad_line, ok ? "ok" : "MISMATCH");
            fails += !ok;
        }
        // a line of exactly the limit is taken
        const std::string fits = head + "7" + mid;
        const std::string text = good + fits + std::string(GS_AS_MAX_LINE - 1 - fits.size(), 'f') + "\n" + good;
        const Result r = run_chunk(text, false, Cfg(), 0);
        gs_host::AsmsumExact exact = exact_of(Cfg());
        exact.feed((const uint8_t *)text.data(), text.size(), false);
        bool ok = !r.refused && r.entries.size() == exact.entries.size();
        for (size_t i = 0; ok && i < r.entries.size(); i++) ok = same(r.entries[i], exact.entries[i]);
        printf("a line of the limit: refused %d entries %zu (want %zu) %s\n", (int)r.refused, r.entries.size(), exact.entries.size(), ok ? "ok" : "MISMATCH");
        fails += !ok;
    }
    // the cap over everything that was kept, at several limits
    const int64_t n = (int64_t)all.size();
    for (int32_t max_per_node : {0, 1, 2, 7, 1000000}) {
        Exact<GsAsmEntry> entries((size_t)n);
        std::string pool_text;
        for (int64_t i = 0; i < n; i++) {
            GsAsmEntry &e = entries.p[i];
            e.node = all[(size_t)i].node;
            e.meta = all[(size_t)i].quality | (uint32_t)all[(size_t)i].is_ref << 8;
            e.line = i;
            e.pool_off = pool_text.size();
            e.len[0] = (uint32_t)all[(size_t)i].taxid.size();
            e.len[1] = (uint32_t)all[(size_t)i].species.size();
            e.len[2] = (uint32_t)all[(size_t)i].ftp.size();
            e.pad = 0;
            pool_text += all[(size_t)i].taxid + all[(size_t)i].species + all[(size_t)i].ftp;
        }
        Exact<uint8_t> pool(pool_text.size());
        memcpy(pool.p, pool_text.data(), pool_text.size());
        const size_t words = KNOWN.size() + 1;
        Exact<uint32_t> node_words(4 * words), seq((size_t)n), seq_alt((size_t)n), perm((size_t)n);
        Exact<u64> key((size_t)n), key_alt((size_t)n), counts(2);
        size_t tmp_bytes = 0;
        gs_asmsum_cap_bytes(n, (int32_t)KNOWN.size(), &tmp_bytes);
        Exact<uint8_t> tmp(tmp_bytes);
        gs_asmsum_cap(entries.p, n, (int32_t)KNOWN.size(), max_per_node, node_words.p, key.p, key_alt.p, seq.p, seq_alt.p, tmp.p, tmp_bytes, perm.p, counts.p, nullptr);
        const size_t m = (size_t)counts.p[0];
        Exact<u64> lens(3 * m + 1), str_off(3 * m + 1);
        Exact<GsAsmEntry> out(m);
        gs_asmsum_pick_sizes(entries.p, perm.p, (int64_t)m, lens.p, str_off.p, tmp.p, tmp_bytes, nullptr);
        Exact<uint8_t> out_pool((size_t)str_off.p[3 * m]);
        gs_asmsum_pick_gather(entries.p, perm.p, (int64_t)m, str_off.p, pool.p, out.p, out_pool.p, nullptr);
        gs_host::AsmsumStore store;
        store.entries = all;
        store.finish(max_per_node);
        bool ok = m == store.picked.size() && counts.p[1] == (u64)store.nodes_with_entries && n > 100;
        for (size_t j = 0; ok && j < m; j++) {
            const gs_host::AsmsumEntry &w = all[store.picked[j]];
            const GsAsmEntry &e = out.p[j];
            ok = perm.p[j] == store.picked[j] && e.node == w.node && e.line == (int64_t)store.picked[j] && e.pool_off == str_off.p[3 * j] &&
                 std::string((const char *)out_pool.p + str_off.p[3 * j], str_off.p[3 * j + 3] - str_off.p[3 * j]) == w.taxid + w.species + w.ftp &&
                 str_off.p[3 * j + 1] - str_off.p[3 * j] == w.taxid.size() && str_off.p[3 * j + 2] - str_off.p[3 * j + 1] == w.species.size();
        }
        printf("cap %d over %lld entries: picked %zu (want %zu) nodes %llu %s\n", max_per_node, (long long)n, m, store.picked.size(), counts.p[1], ok ? "ok" : "MISMATCH");
        fails += !ok;
    }
    printf("fails %d\n", fails);
    return fails != 0;
}
