// gs_sn_walk (genestrip_amd/csrc/gs_snrec.h): what one lane of gs_sn_walk_kernel does for a read that left the match kernel as its
// row of node codes, compiled for the host under AddressSanitizer / UBSan and held to a restatement of the reference's matchRead
// written here in its own terms: per-node vote counts in an array, ancestor tests and sumCounts by walking parent links (no
// pre-order intervals), the error gates as the general loop's double expressions (no table bits), the quotients as divisions.
// Every counter the read adds (seven sums, the max key, four double columns, per node), class and flags are compared, for
//   - 98, 120 and 128 positions,
//   - 1 .. 8 distinct nodes that are an ancestor chain, siblings, unrelated, or drawn at random, as runs in random order with MISS
//     gaps (a node may come back: two contigs, one vote count),
//   - max_paths 1, 2 and 64, thresholds 1 and 3, both error gates off and on,
//   - non-CGAT bytes in the first window, in the middle, in the last window, two and three of them fewer than k apart (the same
//     INVALID windows, different byte counts), and rows of nothing but MISS and INVALID,
// on hand-made trees of 5 and 25 nodes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../genestrip_amd/csrc/gs_snrec.h"

static const int K = 31;
static const int MISS = -1, INVALID = -2, NONE = -3;

struct Tree {
    int n;
    std::vector<int> parent, tin, tout;
};

static Tree make_tree(const std::vector<int> &parent) {
    Tree t;
    t.n = (int)parent.size();
    t.parent = parent;
    t.tin.assign(t.n, 0);
    t.tout.assign(t.n, 0);
    int clock = 0;
    // pre-order numbers by an explicit stack, children in index order
    std::vector<int> stack, next(t.n, 0);
    for (int root = 0; root < t.n; root++) {
        if (parent[root] >= 0) continue;
        stack.push_back(root);
        t.tin[root] = clock++;
        while (!stack.empty()) {
            const int v = stack.back();
            int c = next[v];
            while (c < t.n && parent[c] != v) c++;
            if (c < t.n) {
                next[v] = c + 1;
                t.tin[c] = clock++;
                stack.push_back(c);
            } else {
                t.tout[v] = clock;
                stack.pop_back();
            }
        }
    }
    return t;
}

// 5 nodes: 0 the root, 1 and 2 below it, 3 and 4 below 1
static Tree tree5() { return make_tree({-1, 0, 0, 1, 1}); }
// 25 nodes, five levels: 0; 1 2; 3 4 | 5 6; three species per genus (7 .. 18); strains 19 .. 24 below species 7, 7, 8, 12, 12, 18
static Tree tree25() {
    std::vector<int> p = {-1, 0, 0, 1, 1, 2, 2};
    for (int i = 7; i <= 18; i++) p.push_back(3 + (i - 7) / 3);
    const int strain_of[] = {7, 7, 8, 12, 12, 18};
    for (int s : strain_of) p.push_back(s);
    return make_tree(p);
}

struct Setting {
    int classify, threshold, max_paths;
    double tax, cls;  // max_read_tax_err, max_read_class_err (< 0: off, < 1: a fraction of max, >= 1: a count)
};

struct Tables {
    std::vector<uint64_t> sums, maxk;
    std::vector<double> d;
    explicit Tables(int nv) : sums((size_t)nv * GS_N_SUMS, 0), maxk(nv, 0), d((size_t)nv * GS_N_DCOLS, 0.0) {}
    void add(int vi, int col, uint64_t v) { sums[(size_t)vi * GS_N_SUMS + col] += v; }
    void max_key(int vi, uint64_t key) {
        if (key > maxk[vi]) maxk[vi] = key;
    }
    void dadd(int vi, int col, double v) { d[(size_t)vi * GS_N_DCOLS + col] += v; }
    bool operator==(const Tables &o) const {
        return sums == o.sums && maxk == o.maxk && memcmp(d.data(), o.d.data(), d.size() * sizeof(double)) == 0;
    }
};

static void build_quot(GsQuotTable &T, int max, double m, double mc) {  // the table as launch_batch builds it
    memset(&T, 0, sizeof(T));
    for (int i = 0; i <= max; i++) {
        const double q = (double)i / (double)max;
        T.e[i].q = q;
        T.e[i].q2 = q * q;
        const bool disabled = m >= 0 && ((m >= 1 && (double)i > m) || ((double)i > m * (double)max));
        const bool counted = mc < 0 || (mc >= 1 && (double)i <= mc) || ((double)i <= mc * (double)max);
        if (disabled) T.tax_disabled[i >> 5] |= 1u << (i & 31);
        if (counted) T.class_counted[i >> 5] |= 1u << (i & 31);
    }
}

// ---- the restatement -------------------------------------------------------------------------------
static bool is_anc_or_self(const Tree &t, int a, int x) {  // a on the way from x to the root
    for (; x >= 0; x = t.parent[x])
        if (x == a) return true;
    return false;
}
static int sum_counts(const Tree &t, const std::vector<int> &votes, int x) {  // SmallTaxTree.sumCounts
    int s = 0;
    for (; x >= 0; x = t.parent[x]) s += votes[x];
    return s;
}
static int lca(const Tree &t, int a, int b) {
    if (a < 0 || b < 0) return -1;
    for (; a >= 0; a = t.parent[a])
        if (is_anc_or_self(t, a, b)) return a;
    return -1;
}

// node[p]: the node of position p (value index, MISS or INVALID); bad_bytes: the read's non-CGAT bytes (base indices)
static void restate(const Tree &t, const std::vector<int> &node, const std::vector<int> &bad_bytes, int max, int L, uint32_t r,
                    int64_t first_read_no, const Setting &s, Tables &T, int &cls, int &flags) {
    cls = -1;
    flags = 0;
    const uint64_t m40 = (1ULL << 40) - 1;
    const uint64_t key_lo = m40 - ((uint64_t)(first_read_no + (int64_t)r) & m40);
    std::vector<int> votes(t.n, 0), order;
    int miss = 0, prev = NONE, start = 0;
    bool found = false;
    for (int p = 0; p <= max; p++) {
        const int v = p < max ? node[p] : NONE;
        if (v != prev) {
            if (prev >= 0) {
                const uint64_t len = (uint64_t)(p - start);
                T.add(prev, GS_S_KMERS, len);
                T.add(prev, GS_S_CONTIGS, 1);
                T.add(prev, GS_S_CONTIG_LEN_SQ_SUM, len * len);
                T.max_key(prev, (len << 40) | key_lo);
            }
            prev = v;
            start = p;
        }
        if (v == MISS) miss++;
        if (v >= 0) {
            found = true;
            if (votes[v]++ == 0) order.push_back(v);
        }
    }
    if (!found) return;
    flags = GS_F_FOUND | GS_F_RETURNED;
    std::vector<int> paths;
    for (int v : order) {
        T.add(v, GS_S_READS_1KMER, 1);
        if (!s.classify) continue;
        bool related = false;
        for (size_t i = 0; i < paths.size() && !related; i++) {
            if (is_anc_or_self(t, paths[i], v)) {  // the node lies below the path's end: the path moves down
                paths[i] = v;
                related = true;
            } else if (is_anc_or_self(t, v, paths[i]))
                related = true;
        }
        if (!related && (paths.empty() || (int)paths.size() < s.max_paths)) paths.push_back(v);
    }
    if (!s.classify) return;
    // a non-CGAT byte below position max - 1 costs one error each; any at or behind it cost one together
    int bad_lo = 0;
    bool bad_hi = false;
    for (int b : bad_bytes) {
        if (b < max - 1)
            bad_lo++;
        else
            bad_hi = true;
    }
    const int tax_err = miss + bad_lo + (bad_hi ? 1 : 0);
    if (s.tax >= 0 && ((s.tax >= 1 && (double)tax_err > s.tax) || ((double)tax_err > s.tax * (double)max))) return;
    int best = 0;
    std::vector<int> tied;
    for (int pth : paths) {
        const int sc = sum_counts(t, votes, pth);
        if (sc > best) {
            best = sc;
            tied.clear();
        }
        if (sc >= best) tied.push_back(pth);
    }
    int cn = -1, first_node = -1;
    for (size_t i = 0; i < tied.size(); i++) {
        int x = tied[i];
        if (s.threshold > 1) {  // the lowest node on the way up at which the votes gathered so far reach the threshold
            int acc = 0, mapped = -1;
            for (int y = x; y >= 0 && mapped < 0; y = t.parent[y]) {
                acc += votes[y];
                if (votes[y] > 0 && acc >= s.threshold) mapped = y;
            }
            x = mapped;
        }
        if (i == 0)
            cn = first_node = x;
        else
            cn = cn == x ? cn : lca(t, cn, x);
    }
    cls = cn;
    if (cn < 0) {
        flags &= ~GS_F_RETURNED;
        return;
    }
    const int read_kmers = s.threshold > 1 ? sum_counts(t, votes, first_node) : best;
    const int class_err = max - read_kmers;
    if (!(s.cls < 0 || (s.cls >= 1 && (double)class_err <= s.cls) || ((double)class_err <= s.cls * (double)max))) return;
    flags |= GS_F_COUNTED;
    const double err = (double)tax_err / (double)max, cerr = (double)class_err / (double)max;
    T.add(cn, GS_S_READS, 1);
    T.add(cn, GS_S_READS_KMERS, (uint64_t)read_kmers);
    T.add(cn, GS_S_READS_BPS, (uint64_t)L);
    T.dadd(cn, GS_D_ERR_SUM, err);
    T.dadd(cn, GS_D_ERR_SQ_SUM, err * err);
    T.dadd(cn, GS_D_CLASS_ERR_SUM, cerr);
    T.dadd(cn, GS_D_CLASS_ERR_SQ_SUM, cerr * cerr);
}

// ---- cases -------------------------------------------------------------------------------------------
static uint64_t rng_state = 1;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static int below(int n) { return (int)(rnd() % (uint64_t)n); }

static long long fails = 0, checked = 0, classified = 0;

static void check(const Tree &t, std::vector<int> node, const std::vector<int> &bad_bytes, int max, const Setting &s, const GsQuotTable &Q,
                  const char *what) {
    const int L = max + K - 1;
    // a window that holds a non-CGAT byte is INVALID whatever the store says
    for (int b : bad_bytes)
        for (int p = b - K + 1; p <= b; p++)
            if (p >= 0 && p < max) node[p] = INVALID;
    const uint32_t r = (uint32_t)rnd();
    const int64_t first = (int64_t)(rnd() >> 20);
    Tables want(t.n), got(t.n);
    int wcls, wflags;
    restate(t, node, bad_bytes, max, L, r, first, s, want, wcls, wflags);

    alignas(16) uint16_t codes[GS_SN_ROW];
    for (int p = 0; p < GS_SN_ROW; p++) codes[p] = (uint16_t)(int16_t)(p < max ? node[p] : NONE);
    uint32_t bad = 0;
    bool hi = false;
    for (int b : bad_bytes) {
        if (b < max - 1)
            bad++;
        else
            hi = true;
    }
    bad += hi ? 1u : 0u;
    GsSnWalkConst w;
    w.c.max = max;
    w.c.read_len = L;
    w.c.classify = s.classify;
    w.c.threshold = s.threshold;
    w.max_paths = s.max_paths;
    w.n_values = t.n;
    w.parent = t.parent.data();
    w.tin = t.tin.data();
    w.tout = t.tout.data();
    int32_t cls = -99, flags = -99;
    gs_sn_walk(codes, bad, r, first, w, &Q, got, cls, flags);
    checked++;
    if (wcls >= 0) classified++;
    if (!(want == got) || cls != wcls || flags != wflags) {
        if (fails++ < 10) {
            printf("MISMATCH %s max %d classify %d threshold %d max_paths %d gates %g %g: class %d/%d flags %d/%d tables %s\n  nodes:", what, max,
                   s.classify, s.threshold, s.max_paths, s.tax, s.cls, cls, wcls, flags, wflags, want == got ? "equal" : "differ");
            for (int p = 0; p < max; p++) printf(" %d", node[p]);
            printf("\n");
        }
    }
}

// runs of the given nodes in random order, each node `visits` times, MISS gaps of 0 .. gap positions between them
static std::vector<int> lay_out(const std::vector<int> &nodes, int max, int visits, int gap) {
    std::vector<int> node(max, MISS), seq;
    for (int v = 0; v < visits; v++)
        for (int x : nodes) seq.push_back(x);
    for (size_t i = seq.size(); i > 1; i--) std::swap(seq[i - 1], seq[below((int)i)]);
    int p = below(3) == 0 ? 0 : below(6);
    const int per = max / (int)seq.size();
    for (int x : seq) {
        const int len = 1 + below(per > 1 ? per : 1);
        for (int i = 0; i < len && p < max; i++) node[p++] = x;
        if (gap) p += below(gap + 1);
        if (p >= max) break;
    }
    if (below(2) && !seq.empty())  // the last run reaches the read's end: the tail flush
        for (int q = max - 1 - below(5); q < max; q++) node[q] = seq.back();
    return node;
}

static std::vector<int> pick_nodes(const Tree &t, int kind, int n) {
    std::vector<int> out;
    if (kind == 0) {  // an ancestor chain, from a random deepest node up
        int x = t.n - 1 - below(t.n / 2);
        for (; x >= 0 && (int)out.size() < n; x = t.parent[x]) out.push_back(x);
    } else if (kind == 1) {  // siblings: children of one parent
        for (int tries = 0; tries < 20 && out.size() < 2; tries++) {
            out.clear();
            const int p = below(t.n);
            for (int c = 0; c < t.n && (int)out.size() < n; c++)
                if (t.parent[c] == p) out.push_back(c);
        }
    } else if (kind == 2) {  // unrelated: no one an ancestor of another
        for (int tries = 0; tries < 200 && (int)out.size() < n; tries++) {
            const int x = below(t.n);
            bool ok = true;
            for (int y : out) ok = ok && !is_anc_or_self(t, x, y) && !is_anc_or_self(t, y, x);
            if (ok) out.push_back(x);
        }
    } else {  // anything
        for (int tries = 0; tries < 200 && (int)out.size() < n; tries++) {
            const int x = below(t.n);
            bool ok = true;
            for (int y : out) ok = ok && x != y;
            if (ok) out.push_back(x);
        }
    }
    for (size_t i = out.size(); i > 1; i--) std::swap(out[i - 1], out[below((int)i)]);
    return out;
}

int main() {
    const Tree trees[] = {tree5(), tree25()};
    const int maxes[] = {98, 120, 128};
    std::vector<Setting> settings;
    for (int mp : {1, 2, 64})
        for (int thr : {1, 3})
            for (int gates = 0; gates < 3; gates++)
                settings.push_back({1, thr, mp, gates == 0 ? -1.0 : (gates == 1 ? 0.3 : 40.0), gates == 0 ? -1.0 : (gates == 1 ? 0.6 : 70.0)});
    settings.push_back({0, 1, 64, -1, -1});
    for (const Tree &t : trees)
        for (int max : maxes)
            for (const Setting &s : settings) {
                GsQuotTable Q;
                build_quot(Q, max, s.tax, s.cls);
                rng_state = 77u + (unsigned)max * 131u + (unsigned)t.n;
                const std::vector<int> none;
                for (int kind = 0; kind < 4; kind++)
                    for (int n = 1; n <= 8; n++)
                        for (int rep = 0; rep < 12; rep++) {
                            const std::vector<int> nodes = pick_nodes(t, kind, n);
                            if (nodes.empty()) continue;
                            const std::vector<int> row = lay_out(nodes, max, 1 + rep % 3, rep % 4);
                            check(t, row, none, max, s, Q, "clean");
                            // non-CGAT bytes: the first window, the middle, the last window (bases max - 1 .. L - 1), and groups
                            // fewer than k apart whose windows are one INVALID stretch
                            check(t, row, {below(K)}, max, s, Q, "bad byte in the first window");
                            check(t, row, {max / 2 + below(9)}, max, s, Q, "bad byte in the middle");
                            check(t, row, {max - 1 + below(K)}, max, s, Q, "bad byte in the last window");
                            check(t, row, {max - 2}, max, s, Q, "bad byte in front of the last window");
                            check(t, row, {40, 42}, max, s, Q, "two bad bytes");
                            check(t, row, {40, 41, 42}, max, s, Q, "three bad bytes, the same windows");
                            check(t, row, {0, max / 2, max + K - 2}, max, s, Q, "bad bytes at both ends and in the middle");
                        }
                // rows without a hit: nothing but MISS, nothing but INVALID, both
                std::vector<int> all_miss(max, MISS);
                check(t, all_miss, none, max, s, Q, "all MISS");
                check(t, all_miss, {5}, max, s, Q, "MISS and INVALID");
                std::vector<int> every;
                for (int b = 0; b < max + K - 1; b += K) every.push_back(b);
                check(t, all_miss, every, max, s, Q, "all INVALID");
                // one node on every position, and alone on the first and on the last
                std::vector<int> full(max, t.n - 1), first_only(max, MISS), last_only(max, MISS);
                first_only[0] = 1;
                last_only[max - 1] = 2;
                check(t, full, none, max, s, Q, "one node everywhere");
                check(t, first_only, none, max, s, Q, "one hit at position 0");
                check(t, last_only, none, max, s, Q, "one hit at position max - 1");
                // as many distinct nodes as the tree has, one position each, twice over
                std::vector<int> many(max, MISS);
                for (int p = 0; p < max && p < 2 * t.n; p++) many[p] = p % t.n;
                check(t, many, none, max, s, Q, "every node of the tree");
            }
    printf("checked %lld reads (%lld classified), fails %lld\n", checked, classified, fails);
    return fails ? 1 : 0;
}
