// gs_taxparse.h -- the taxtree and taxnodes goals line by line, as the reference does them: TaxTree(File, boolean)
// (C/tax/TaxTree.java:92-122, readNodesFromStream :226-254, readNamesFromStream :196-216, initPositions :491-502) over the lines of
// BufferedLineReader.nextLine (B/io/BufferedLineReader.java:160-182) and the keys of DigitTrie (C/util/DigitTrie.java:106-189);
// TaxIdCollector (C/tax/TaxIdCollector.java:67-126,172-185) under TaxNodesGoal (C/goals/TaxNodesGoal.java:74-94);
// TaxIdNode.markRequired (TaxTree.java:536-544), SmallTaxTree(TaxTree) (C/tax/SmallTaxTree.java:60-64,427-454) and
// Database.initStoreIndices (C/store/Database.java:107-128) on a store that has no values yet.  Pure host code without a device call
// or a thread.  The gs_taxtree handle (gs_api.cpp) feeds it what the device refuses (gs_taxtree.hip), every names line, and
// everything on a host-only handle.
//
// Kept as the reference has it:
//   * a line is what nextLine puts into its 4096-byte target: NUL bytes dropped, '\r' kept, the newline a part of it, the last
//     line of a stream with or without one.  A line that fills the target answers 4097 and ITS REST IS READ AS THE NEXT LINE; the
//     searches then run to index 4096 and throw if they find nothing in front of it.  The stream ends at the first size 0.
//   * nodes: a, b, c are the first three '|', each searched for behind the one before (from 0 again behind a -1).  Without a or b the
//     line is skipped.  id is [0, a-1), parent [a+2, b-1), rank [b+2, c-1): the byte in front of a bar is dropped unseen.  Both
//     trie gets CREATE: a byte that is no digit throws (IllegalStateException), a key of negative length throws
//     (StringIndexOutOfBoundsException).  A parent that no line introduces is a node: rank none, no parent.  A child joins its
//     parent's list in line order -- once per line, so two lines with one id list it twice, and its parent is the last one named.
//     id == parent adds no child.  The rank is the ordinal of the Rank whose name equals the field, else -1.  The root is the node
//     "1" of a line whose id and parent are both "1".
//   * names: the node is looked up without create: an unknown id, or one with a byte that is no digit, skips the line.  The name
//     is [a+2, b-1) (negative length: throws); it is taken if the node has none yet or the LINE holds "scientific name" anywhere.
//   * initPositions(0, 0) from the root: depth and pre-order position, children in list order.  What the root does not reach
//     keeps depth -1, position -1, subtree 0.  A cycle that the root reaches never ends there (StackOverflowError): it fails here.
//   * completeFilterlist adds its start node and descends child lists, whether the root reaches them or not; into a child only if
//     the cut is null or the child has a rank that is not below it.  A start node on a cycle never ends: it fails here.
// NOT as the reference has it: it keys a node by the STRING of its id, so "01", "" (a bar in column 1) and ids beyond int32 are
// nodes of their own there.  A node is an int32 tax id in this library: such an id FAILS with code 2 (unsupported), as does an id
// of more than nine digits.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace gs_host {

enum { TAX_MAX_LINE = 4096, TAX_N_RANKS = 40 };
static const char *const TAX_RANK_NAMES[TAX_N_RANKS] = {
    "cellular root", "acellular root", "superkingdom", "domain", "realm", "kingdom", "phylum", "subphylum", "superclass", "class",
    "subclass", "superorder", "order", "suborder", "superfamily", "family", "subfamily", "tribe", "genus", "subgenus",
    "species group", "species", "varietas", "subspecies", "serogroup", "biotype", "strain", "serotype", "genotype", "forma",
    "forma specialis", "isolate", "clade", "no rank", "subkingdom", "section", "REFINED", "DATA", "FILE", "ID"};

// Rank.level: ordinal * 20; clade and no rank: -1; subkingdom: kingdom + 10; section: genus + 10 (C/tax/Rank.java:104-112,176-184)
static inline int tax_rank_level(int ordinal) {
    if (ordinal == 32 || ordinal == 33) return -1;
    if (ordinal == 34) return 5 * 20 + 10;
    if (ordinal == 35) return 18 * 20 + 10;
    return ordinal * 20;
}
// Rank.isBelow over ordinals (:227-256)
static inline bool tax_rank_below(int rank, int other) {
    const int a = tax_rank_level(rank), b = tax_rank_level(other);
    return a != -1 && b != -1 && a > b;
}

// what decides among the names lines of a node, whoever judged them: the highest key.  A scientific line with its 1-based line number
// is above every other line (a later one replaces an earlier one); among the others the first line wins
static inline uint64_t tax_name_key(bool scientific, int64_t line) {
    return scientific ? (1ull << 63) | (uint64_t)line : 0x7fffffffffffffffull - (uint64_t)line;
}

struct TaxSlot {
    int32_t id, parent, rank, pad;  // id 0: an empty slot (a line that is skipped)
};

struct TaxError {
    int code = 0;  // 1: the reference throws; 2: unsupported here
    int64_t line = 0;
    std::string what;
};

// the lines of one stream; whole lines come in through feed()
struct TaxLines {
    uint8_t target[TAX_MAX_LINE];
    int64_t line_no = 0;
    TaxError err;

    bool fail(int code, const char *what) {
        err.code = code;
        err.line = line_no;
        err.what = what;
        return false;
    }
    // ByteArrayUtil.indexOf(target, start, size, c); -2: it reads target[4096]
    int index_of(int start, int size, uint8_t c) const {
        for (int i = start; i < size; i++) {
            if (i >= TAX_MAX_LINE) return -2;
            if (target[i] == c) return i;
        }
        return -1;
    }
    // the key target[start, end) as a tax id.  > 0: the id; 0: no node can have this key; -1: failed (create only)
    int32_t taxid(int start, int end, bool create) {
        if (end < start) {
            if (create) fail(1, "a key of negative length (StringIndexOutOfBoundsException)");
            return create ? -1 : 0;
        }
        for (int i = start; i < end; i++)
            if (target[i] < '0' || target[i] > '9') {
                if (create) fail(1, "Cant get node via sequence (IllegalStateException): a byte that is no digit");
                return create ? -1 : 0;
            }
        if (end == start || target[start] == '0' || end - start > 9) {
            if (create) fail(2, "an empty tax id, a leading zero or more than nine digits: the reference makes a node that an int32 tax id cannot name");
            return create ? -1 : 0;
        }
        int32_t v = 0;
        for (int i = start; i < end; i++) v = v * 10 + (target[i] - '0');
        return v;
    }
    // nextLine over [*p, end): the size it answers, *p behind what it consumed
    int next_line(const uint8_t **p, const uint8_t *end) {
        int size = 0;
        uint8_t c = 0xff;
        const uint8_t *q = *p;
        while (size < TAX_MAX_LINE && q < end && c != '\n') {
            c = *q++;
            if (c != 0) target[size++] = c;
        }
        *p = q;
        if (c == '\n') return size;
        if (size == TAX_MAX_LINE) return size + 1;
        return size;
    }
};

struct TaxNodesExact : TaxLines {
    std::vector<TaxSlot> slots;  // one per line that is not skipped, in input order

    // [p, p + n): whole lines; last: the stream ends behind them.  false: err says why, err.line is the 1-based line
    bool feed(const uint8_t *p, size_t n, bool last) {
        const uint8_t *end = p + n;
        if (!last && n && end[-1] != '\n') {
            line_no++;
            return fail(1, "a chunk that is not the last ends inside a line");
        }
        while (p < end) {
            const int size = next_line(&p, end);
            if (size == 0) break;
            line_no++;
            const int a = index_of(0, size, '|');
            const int b = a == -2 ? -2 : index_of(a + 1, size, '|');
            const int c = b == -2 ? -2 : index_of(b + 1, size, '|');
            if (c == -2) return fail(1, "no bar in a line that fills the buffer (ArrayIndexOutOfBoundsException)");
            if (a == -1 || b == -1) continue;
            TaxSlot s;
            if ((s.id = taxid(0, a - 1, true)) < 0) return false;
            if ((s.parent = taxid(a + 2, b - 1, true)) < 0) return false;
            s.rank = -1;
            s.pad = 0;
            const int len = c - 1 - (b + 2);
            for (int r = 0; r < TAX_N_RANKS && len >= 0; r++)
                if ((int)strlen(TAX_RANK_NAMES[r]) == len && memcmp(TAX_RANK_NAMES[r], target + b + 2, (size_t)len) == 0) {
                    s.rank = r;
                    break;
                }
            slots.push_back(s);
        }
        return true;
    }
};

// TaxIdNode.incRefSeqRegions (C/tax/TaxTree.java:517-521) without the node itself: regions[v] of every node v -- with `only`, of
// every node with only[v] < 0 -- is added to incl[u] for each u above v on its parent chain (mod 2^32).  false: a node with
// regions stands on or below a cycle of parent links, where the reference's walk does not end
inline bool tax_regions_up(const int32_t *parent, int32_t n, const int32_t *regions, const int32_t *only, int32_t *incl) {
    for (int32_t v = 0; v < n; v++) {
        if (regions[(size_t)v] == 0 || (only && only[(size_t)v] >= 0)) continue;
        int32_t steps = 0;
        for (int32_t u = parent[(size_t)v]; u != -1; u = parent[(size_t)u]) {
            if (steps++ >= n) return false;
            incl[(size_t)u] = (int32_t)((uint32_t)incl[(size_t)u] + (uint32_t)regions[(size_t)v]);
        }
    }
    return true;
}

// TaxNodesFromGenbankGoal's loop (C/goals/genbank/TaxNodesFromGenbankGoal.java:86-92) over node indices: the selected nodes of the
// rank asked for (check_rank < 0: any) whose count is below limit, once each, ascending
inline void tax_regions_below(const int32_t *incl, const int32_t *rank, int32_t n, const int32_t *selected, int64_t n_sel, int32_t limit, int check_rank,
                              std::vector<int32_t> &below) {
    std::vector<uint8_t> marks((size_t)n, 0);
    for (int64_t i = 0; i < n_sel; i++) marks[(size_t)selected[i]] = 1;
    below.clear();
    for (int32_t v = 0; v < n; v++)
        if (marks[(size_t)v] && (check_rank < 0 || rank[(size_t)v] == check_rank) && incl[(size_t)v] < limit) below.push_back(v);
}

// the tree over slots, with the reference's literal child lists
struct TaxHostTree {
    int32_t n = 0, root = -1;
    int64_t duplicates = 0;
    std::vector<int32_t> taxids, parent, rank, depth, position, subtree;
    std::vector<int64_t> child_off;  // n + 1
    std::vector<int32_t> child;      // the lists back to back, each in line order
    std::vector<std::string> names;
    std::vector<uint8_t> has_name;
    std::vector<uint64_t> name_key;  // per node: the key of the line its name came from (tax_name_key); 0: none

    int32_t node_of(int32_t taxid) const {
        auto it = std::lower_bound(taxids.begin(), taxids.end(), taxid);
        return it != taxids.end() && *it == taxid ? (int32_t)(it - taxids.begin()) : -1;
    }

    // false: why says it (no root; a cycle under the root)
    bool build(const TaxSlot *slots, size_t m, std::string *why) {
        taxids.clear();
        taxids.reserve(2 * m);
        for (size_t i = 0; i < m; i++)
            if (slots[i].id > 0) {
                taxids.push_back(slots[i].id);
                taxids.push_back(slots[i].parent);
            }
        std::sort(taxids.begin(), taxids.end());
        taxids.erase(std::unique(taxids.begin(), taxids.end()), taxids.end());
        n = (int32_t)taxids.size();
        parent.assign((size_t)n, -1);
        rank.assign((size_t)n, -1);
        depth.assign((size_t)n, -1);
        position.assign((size_t)n, -1);
        subtree.assign((size_t)n, 0);
        names.assign((size_t)n, std::string());
        has_name.assign((size_t)n, 0);
        name_key.assign((size_t)n, 0);
        child_off.assign((size_t)n + 1, 0);
        std::vector<uint8_t> seen((size_t)n, 0);
        std::vector<int32_t> a_of(m, -1), b_of(m, -1);
        root = -1;
        duplicates = 0;
        for (size_t i = 0; i < m; i++) {
            if (slots[i].id <= 0) continue;
            const int32_t a = node_of(slots[i].id), b = node_of(slots[i].parent);
            a_of[i] = a;
            b_of[i] = b;
            duplicates += seen[(size_t)a];
            seen[(size_t)a] = 1;
            if (a != b) {
                child_off[(size_t)b + 1]++;
                parent[(size_t)a] = b;
            }
            rank[(size_t)a] = slots[i].rank;
            if (a == b && slots[i].id == 1) root = a;
        }
        for (int32_t v = 0; v < n; v++) child_off[(size_t)v + 1] += child_off[(size_t)v];
        child.assign((size_t)child_off[(size_t)n], -1);
        std::vector<int64_t> fill(child_off.begin(), child_off.end() - 1);
        for (size_t i = 0; i < m; i++)
            if (a_of[i] >= 0 && a_of[i] != b_of[i]) child[(size_t)fill[(size_t)b_of[i]]++] = a_of[i];
        if (root < 0) {
            *why = "no root: no line has the id 1 and the parent 1";
            return false;
        }
        // initPositions(0, 0) without the recursion
        std::vector<int32_t> stack;
        std::vector<int64_t> next;
        std::vector<uint8_t> on_stack((size_t)n, 0);
        int32_t counter = 0;
        position[(size_t)root] = 0;
        depth[(size_t)root] = 0;
        stack.push_back(root);
        next.push_back(child_off[(size_t)root]);
        on_stack[(size_t)root] = 1;
        while (!stack.empty()) {
            const int32_t v = stack.back();
            if (next.back() < child_off[(size_t)v + 1]) {
                const int32_t c = child[(size_t)next.back()++];
                if (on_stack[(size_t)c]) {
                    *why = "the root reaches a cycle: the reference's initPositions does not end";
                    return false;
                }
                if (counter == INT32_MAX) {
                    *why = "more than 2^31 visits";
                    return false;
                }
                position[(size_t)c] = ++counter;
                depth[(size_t)c] = (int32_t)stack.size();
                stack.push_back(c);
                next.push_back(child_off[(size_t)c]);
                on_stack[(size_t)c] = 1;
            } else {
                subtree[(size_t)v] = counter - position[(size_t)v] + 1;
                on_stack[(size_t)v] = 0;
                stack.pop_back();
                next.pop_back();
            }
        }
        return true;
    }

    // withDescendants(starts, cut) into res (uint8[n], or-ed); cut: a rank ordinal or -1.  false: a start node reaches a cycle
    bool complete(const int32_t *starts, int64_t n_starts, int cut, uint8_t *res) const {
        std::vector<int32_t> stack;
        std::vector<int64_t> next;
        std::vector<uint8_t> on_stack((size_t)n, 0);
        for (int64_t s = 0; s < n_starts; s++) {
            // (what an earlier start has entered is entered again: whether the descent passes depends on the child alone, but a
            // cycle must be met on the stack)
            stack.assign(1, starts[s]);
            next.assign(1, child_off[(size_t)starts[s]]);
            on_stack[(size_t)starts[s]] = 1;
            res[(size_t)starts[s]] = 1;
            while (!stack.empty()) {
                const int32_t v = stack.back();
                if (next.back() < child_off[(size_t)v + 1]) {
                    const int32_t c = child[(size_t)next.back()++];
                    if (cut >= 0 && (rank[(size_t)c] < 0 || tax_rank_below(rank[(size_t)c], cut))) continue;
                    if (on_stack[(size_t)c]) return false;
                    if (res[(size_t)c] == 2) continue;  // left before, by this call: no cycle below it
                    res[(size_t)c] = 1;
                    stack.push_back(c);
                    next.push_back(child_off[(size_t)c]);
                    on_stack[(size_t)c] = 1;
                } else {
                    res[(size_t)v] = 2;
                    on_stack[(size_t)v] = 0;
                    stack.pop_back();
                    next.pop_back();
                }
            }
        }
        for (int32_t v = 0; v < n; v++) res[(size_t)v] = res[(size_t)v] != 0;
        return true;
    }

    // TaxNodesGoal.doMakeThis over node indices -> out[n]
    bool select(const int32_t *requested, int64_t n_req, const int32_t *excluded, int64_t n_exc, int cut, uint8_t *out) const {
        std::vector<uint8_t> ex((size_t)n, 0);
        memset(out, 0, (size_t)n);
        if (!complete(requested, n_req, cut, out) || !complete(excluded, n_exc, -1, ex.data())) return false;
        for (int32_t v = 0; v < n; v++) out[(size_t)v] = out[(size_t)v] && !ex[(size_t)v];
        return true;
    }

    // markRequired per flagged node, SmallTaxTree(TaxTree), initStoreIndices: the root is always in; one value index per node
    template <class Flag>
    void small(const Flag *flagged, std::vector<int32_t> &node_of_vi, std::vector<int32_t> &parent_vi) const {
        std::vector<uint8_t> required((size_t)n, 0);
        for (int32_t f = 0; f < n; f++)
            if (flagged[f] > 0)
                for (int32_t v = f; v != -1 && !required[(size_t)v]; v = parent[(size_t)v]) required[(size_t)v] = 1;
        std::vector<int32_t> vi((size_t)n, -1), stack;
        std::vector<int64_t> next;
        node_of_vi.assign(1, root);
        parent_vi.assign(1, -1);
        vi[(size_t)root] = 0;
        stack.push_back(root);
        next.push_back(child_off[(size_t)root]);
        while (!stack.empty()) {
            const int32_t v = stack.back();
            if (next.back() < child_off[(size_t)v + 1]) {
                const int32_t c = child[(size_t)next.back()++];
                if (!required[(size_t)c] || vi[(size_t)c] >= 0) continue;
                vi[(size_t)c] = (int32_t)node_of_vi.size();
                node_of_vi.push_back(c);
                parent_vi.push_back(vi[(size_t)v]);
                stack.push_back(c);
                next.push_back(child_off[(size_t)c]);
            } else {
                stack.pop_back();
                next.pop_back();
            }
        }
    }
};

// readNamesFromStream over whole lines, into a built tree
struct TaxNamesExact : TaxLines {
    bool feed(TaxHostTree &t, const uint8_t *p, size_t n, bool last) {
        const uint8_t *end = p + n;
        if (!last && n && end[-1] != '\n') {
            line_no++;
            return fail(1, "a chunk that is not the last ends inside a line");
        }
        static const char pat[] = "scientific name";
        const int plen = (int)sizeof(pat) - 1;
        while (p < end) {
            const int size = next_line(&p, end);
            if (size == 0) break;
            line_no++;
            bool scientific = false;
            for (int i = 0; i <= size - plen && !scientific; i++) {
                int j = 0;
                while (j < plen) {
                    if (i + j >= TAX_MAX_LINE) return fail(1, "the search for the scientific name reads behind the buffer (ArrayIndexOutOfBoundsException)");
                    if (target[i + j] != (uint8_t)pat[j]) break;
                    j++;
                }
                scientific = j == plen;
            }
            const int a = index_of(0, size, '|');
            const int b = a == -2 ? -2 : index_of(a + 1, size, '|');
            if (b == -2) return fail(1, "no bar in a line that fills the buffer (ArrayIndexOutOfBoundsException)");
            if (a == -1 || b == -1) continue;
            const int32_t id = taxid(0, a - 1, false);
            const int32_t node = id > 0 ? t.node_of(id) : -1;
            if (node < 0) continue;
            if (b - a - 3 < 0) return fail(1, "a name of negative length (StringIndexOutOfBoundsException)");
            if (!t.has_name[(size_t)node] || scientific) {
                t.names[(size_t)node].assign((const char *)target + a + 2, (size_t)(b - a - 3));
                t.has_name[(size_t)node] = 1;
                t.name_key[(size_t)node] = tax_name_key(scientific, line_no);
            }
        }
        return true;
    }
};

// TaxIdCollector.readFromFile, the strings alone: lines end at \n, \r or \r\n; trimmed as String.trim does; '#' starts a comment;
// the value is what follows the last tab; a leading '-' excludes.  The ids that are 1-9 digits without a leading zero come back as
// numbers (any other string names no node here and is dropped)
static inline void tax_read_taxids(const uint8_t *p, size_t n, std::vector<int32_t> &requested, std::vector<int32_t> &excluded) {
    auto trim = [](const uint8_t *&a, const uint8_t *&b) {
        while (a < b && *a <= ' ') a++;
        while (b > a && b[-1] <= ' ') b--;
    };
    const uint8_t *end = p + n;
    while (p < end) {
        const uint8_t *e = p;
        while (e < end && *e != '\n' && *e != '\r') e++;
        const uint8_t *a = p, *b = e;
        p = e < end ? e + 1 : end;
        trim(a, b);
        if (a < b && *a == '#') continue;
        const uint8_t *hash = (const uint8_t *)memchr(a, '#', (size_t)(b - a));
        if (hash) b = hash;
        for (const uint8_t *t = b; t > a; t--)
            if (t[-1] == '\t') {
                a = t - 1;
                break;
            }
        trim(a, b);
        if (a == b) continue;
        const bool minus = *a == '-';
        if (minus) a++;
        if (b - a < 1 || b - a > 9 || *a == '0') continue;
        int32_t v = 0;
        bool ok = true;
        for (const uint8_t *t = a; t < b; t++) {
            ok = ok && *t >= '0' && *t <= '9';
            v = v * 10 + (*t - '0');
        }
        if (ok) (minus ? excluded : requested).push_back(v);
    }
}

}  // namespace gs_host
