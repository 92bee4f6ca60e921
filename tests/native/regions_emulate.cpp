// regions_emulate.cpp -- the regions kernels of genestrip_amd/csrc/gs_taxtree.hip (scatter to pre-order, scan, difference; mark, flag,
// scan, compaction) compiled for the host against the stand-in of taxtree_emulate.cpp and run under AddressSanitizer / UBSan, every
// array exactly as large as gs_taxtree_regions_below makes it at the least (pre, sum: one word per reached node; incl, flag, idx,
// out: one per node; marks: one byte per node; the selection).  What comes out is held to the parent walk of gs_taxparse.h.
// Trees, scan and finish are those of taxtree_emulate.cpp, whose main is set aside.
#define main taxtree_emulate_main
#include "taxtree_emulate.cpp"
#undef main

int main() {
    for (int r = 0; r < GS_TT_N_RANKS; r++) {
        g_ranks.len[r] = (uint8_t)strlen(TAX_RANK_NAMES[r]);
        memcpy(g_ranks.text[r], TAX_RANK_NAMES[r], g_ranks.len[r]);
    }
    static const char *ranks[] = {"no rank", "species", "genus", "strain", "odd"};
    std::mt19937_64 rng(11);
    // node counts around the block of 256 and the wave of 64, and one of several blocks
    for (int n : {1, 63, 64, 256, 257, 700}) {
        std::vector<std::string> lines;
        lines.push_back(node_line(1, 1, "no rank", 0));
        for (int i = 2; i <= n; i++) lines.push_back(node_line(i * 3, i == 2 || rng() % 8 == 0 ? 1 : (int)(2 + rng() % (i - 2)) * 3, ranks[rng() % 5], 0));
        if (n != 64 && n != 256) {  // what the root does not reach; without it at 64 and 256 the arrays end with a full wave and block
            lines.push_back(node_line(5000, 7777, "species", 0));
            lines.push_back(node_line(5001, 5000, "strain", 0));
            lines.push_back(node_line(6001, 6001, "no rank", 0));
            lines.push_back(node_line(6002, 6001, "species", 0));
            lines.push_back(node_line(8000, 8002, "genus", 0));  // a two-cycle with a tail: it gets no regions
            lines.push_back(node_line(8002, 8000, "genus", 0));
            lines.push_back(node_line(8004, 8002, "species", 0));
        }
        std::shuffle(lines.begin(), lines.end(), rng);
        std::string text;
        for (auto &l : lines) text += l;
        std::vector<TaxSlot> slots;
        uint32_t bad = 0;
        CHECK(scan_nodes(text, true, slots, &bad));
        DeviceTree t;
        CHECK(finish(slots, t));
        const size_t N = (size_t)t.n, R = (size_t)t.n_reach;
        CHECK(n == 64 || n == 256 ? R == N && N == (size_t)n : R + 8 == N);
        for (int turn = 0; turn < 3; turn++) {
            std::vector<int32_t> regions(N), selected;
            for (size_t v = 0; v < N; v++) {
                const bool cyc = t.taxids[v] >= 8000 && t.taxids[v] <= 8004;
                regions[v] = !cyc && rng() % 3 == 0 ? 1 + (int32_t)(rng() % 50) : 0;
                if (turn == 0 || rng() % 2) selected.push_back((int32_t)v);
                if (rng() % 5 == 0) selected.push_back((int32_t)v);  // a node twice
            }
            if (turn == 1) selected.clear();
            std::shuffle(selected.begin(), selected.end(), rng);
            const size_t S = selected.size();
            const int32_t limit = turn == 0 ? INT32_MAX : 40;
            const int check_rank = turn == 2 ? 21 : -1;  // species
            // the host's answer
            std::vector<int32_t> want(regions), below;
            CHECK(tax_regions_up(t.parent.data(), t.n, regions.data(), nullptr, want.data()));
            tax_regions_below(want.data(), t.rank.data(), t.n, selected.data(), (int64_t)S, limit, check_rank, below);
            // the device's, with the parent walk for what the root does not reach in between, as gs_taxtree_regions_below has it
            size_t tmp_bytes = 0;
            gs_taxtree_sort_bytes((int64_t)N, &tmp_bytes);
            Exact<uint8_t> tmp(tmp_bytes), marks(N);
            Exact<uint32_t> pre(R), sum(R), flag(N), idx(N);
            Exact<int32_t> d_regions(N), incl(N), out(N), d_sel(S);
            memcpy(d_regions.p, regions.data(), N * sizeof(int32_t));
            if (S) memcpy(d_sel.p, selected.data(), S * sizeof(int32_t));
            gs_launch_taxtree_regions(&t.A, t.n_reach, d_regions.p, pre.p, sum.p, tmp.p, tmp_bytes, incl.p, nullptr);
            if (R < N) {
                const std::vector<int32_t> own(incl.p, incl.p + N);
                CHECK(tax_regions_up(t.parent.data(), t.n, own.data(), t.position.data(), incl.p));
            }
            CHECK(memcmp(incl.p, want.data(), N * sizeof(int32_t)) == 0);
            gs_launch_taxtree_below(&t.A, d_sel.p, (int64_t)S, incl.p, limit, check_rank, marks.p, flag.p, idx.p, tmp.p, tmp_bytes, out.p, nullptr);
            const size_t count = (size_t)flag.p[N - 1] + idx.p[N - 1];
            CHECK(count == below.size());
            CHECK(count <= N && (count == 0 || memcmp(out.p, below.data(), count * sizeof(int32_t)) == 0));
            if (turn == 0) CHECK(count == N);  // every node, each once
            if (turn == 1) CHECK(count == 0);
        }
        // regions on the tail of the cycle: the walk must say so and stop
        if (R < N) {
            std::vector<int32_t> regions(N, 0), incl(N, 0);
            for (size_t v = 0; v < N; v++) regions[v] = t.taxids[v] == 8004;
            CHECK(!tax_regions_up(t.parent.data(), t.n, regions.data(), t.position.data(), incl.data()));
        }
        printf("nodes %d %s\n", n, fails ? "MISMATCH" : "ok");
    }
    printf("fails %d\n", fails);
    return fails != 0;
}
