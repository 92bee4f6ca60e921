// gs_asmsumparse.h -- the fastasgenbank goal record by record, as the reference does it: AssemblySummaryReader.getRelevantEntries
// (C/genbank/AssemblySummaryReader.java:104-144) over the records of Commons CSV 1.9.0 (quote = null, comment marker '#', delimiter
// TAB, ignoreEmptyLines, no escape, no trimming, the bytes decoded as UTF-8), AssemblyEntry's file name (:170-192),
// AssemblyQuality.fromString (:294-308), the node of a tax id string (C/tax/TaxTree.java:367-369 over C/util/DigitTrie.java:192-225)
// and the cap of FastaFilesFromGenbankGoal (C/goals/genbank/FastaFilesFromGenbankGoal.java:101-150).  Pure host code without a
// device call or a thread: tests/native/asmsumparse_sanitize.cpp runs it on its own.  gs_host_asmsum_files (gs_host.cpp) feeds it
// what the device refuses (gs_asmsum.hip), lines that do not fit a reader block, the unterminated tail of a file, and whole files
// under GS_HOST_FAST=0.  The host-only handle of gs_api.cpp (device -1) keeps its entries in AsmsumStore.
//
// The rules:
//   * a line ends at LF, at CR, or at CR LF (one terminator), or at the end of the stream; the last line need not be terminated.
//     Every line has a number, 0-based, whatever it holds.
//   * an empty line is no record; a line whose first byte is '#' is no record.  NUL bytes are ordinary bytes.
//   * a record has tabs + 1 fields; one with fewer than 20 is skipped and not counted, every other one counts.
//   * the key is field 6 (use_species) or field 5; its UTF-16 units are cut to their low bytes (DigitTrie: (byte) charAt(i)), so
//     U+0131 reads as '1'.  A non-digit gives no node, "007" is not 7, the empty key gives no node.
//   * filter, quality (field 11 with field 10 == "latest"), reference (field 4 == "reference genome"), in this order.
//   * a kept entry with an EMPTY ftp field (field 19) throws in the reference: feed() fails and names the 1-based line.
// feed() takes the stream in pieces of any size: a partial line and a CR at the end of a piece carry over.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace gs_host {

struct AsmsumEntry {
    int32_t node;
    uint8_t quality, is_ref;
    int64_t line;  // 0-based, of the whole stream
    std::string taxid, species, ftp;
};

// AssemblyQuality's ordinal of (assembly level, version status)
inline int asmsum_quality(const uint8_t *level, size_t n_level, const uint8_t *status, size_t n_status) {
    const bool latest = n_status == 6 && memcmp(status, "latest", 6) == 0;
    static const char *const names[4] = {"Complete Genome", "Chromosome", "Scaffold", "Contig"};
    for (int i = 0; i < 4; i++)
        if (n_level == strlen(names[i]) && memcmp(level, names[i], n_level) == 0) return 2 * i + (latest ? 1 : 2);
    return latest ? 9 : 10;
}

// the base of AssemblyEntry's file name: [*from, *to) of ftp[0 .. n); n == 0 is the caller's to refuse
inline void asmsum_base_name(const uint8_t *ftp, size_t n, size_t *from, size_t *to) {
    int64_t pos = -1;
    for (int64_t i = (int64_t)n - 1; i >= 0 && pos < 0; i--)
        if (ftp[i] == '/') pos = i;
    if (pos == (int64_t)n - 1) {
        int64_t prev = -1;
        for (int64_t i = pos - 1; i >= 0 && prev < 0; i--)
            if (ftp[i] == '/') prev = i;
        *from = (size_t)(prev + 1);
        *to = n - 1;
    } else {
        *from = (size_t)(pos + 1);
        *to = n;
    }
}

// the units of a Java String made from these bytes by the UTF-8 decoder, each cut to its low byte.  Malformed input gives
// U+FFFD there, however many of them: here one 0xFD per malformed byte -- no digit either way
inline std::string asmsum_low_bytes(const uint8_t *p, size_t n) {
    std::string out;
    for (size_t i = 0; i < n;) {
        const uint32_t b = p[i];
        if (b < 0x80) {
            out.push_back((char)b);
            i++;
            continue;
        }
        int more = b >= 0xc2 && b <= 0xdf ? 1 : b >= 0xe0 && b <= 0xef ? 2 : b >= 0xf0 && b <= 0xf4 ? 3 : -1;
        uint32_t cp = more == 1 ? b & 0x1f : more == 2 ? b & 0x0f : b & 0x07;
        bool ok = more > 0 && i + (size_t)more < n;
        for (int j = 1; ok && j <= more; j++) {
            ok = (p[i + (size_t)j] & 0xc0) == 0x80;
            cp = cp << 6 | (p[i + (size_t)j] & 0x3f);
        }
        if (ok && more == 2) ok = cp >= 0x800 && !(cp >= 0xd800 && cp <= 0xdfff);
        if (ok && more == 3) ok = cp >= 0x10000 && cp <= 0x10ffff;
        if (!ok) {
            out.push_back((char)0xfd);
            i++;
            continue;
        }
        if (cp >= 0x10000) {  // a surrogate pair: two units
            cp -= 0x10000;
            out.push_back((char)((0xd800 + (cp >> 10)) & 0xff));
            out.push_back((char)((0xdc00 + (cp & 0x3ff)) & 0xff));
        } else {
            out.push_back((char)(cp & 0xff));
        }
        i += (size_t)more + 1;
    }
    return out;
}

struct AsmsumExact {
    std::vector<int32_t> known;   // ascending, distinct, positive: a node is an index into it
    std::vector<uint8_t> filter;  // known.size() flags; empty: every node
    int32_t quality_mask = -1;    // bit q: ordinal q allowed
    bool reference_only = false, use_species = false;

    std::vector<AsmsumEntry> entries;  // in input order
    int64_t counted = 0, short_records = 0, skipped = 0;  // records of 20 fields and more; of fewer; comment and empty lines
    int64_t line_no = 0;  // lines of the stream seen so far, wherever they were judged
    std::string error;    // why feed() failed: on line line_no (1-based: the line has been counted)

    void begin_stream() {
        line_no = 0;
        pending_.clear();
        has_pending_ = skip_lf_ = false;
    }

    // the next bytes of the stream; last: it ends behind them.  false: the reference throws on line line_no
    bool feed(const uint8_t *p, size_t n, bool last) {
        const uint8_t *end = p + n;
        if (skip_lf_ && p < end) {
            if (*p == '\n') p++;
            skip_lf_ = false;
        }
        while (p < end) {
            const uint8_t *q = p;
            while (q < end && *q != '\n' && *q != '\r') q++;
            if (q == end) {  // no terminator yet
                pending_.append((const char *)p, (size_t)(q - p));
                has_pending_ = true;
                break;
            }
            bool ok;
            if (has_pending_) {
                pending_.append((const char *)p, (size_t)(q - p));
                ok = line((const uint8_t *)pending_.data(), pending_.size());
                pending_.clear();
                has_pending_ = false;
            } else {
                ok = line(p, (size_t)(q - p));
            }
            if (!ok) return false;
            p = q + 1;
            if (*q == '\r') {
                if (p < end) {
                    if (*p == '\n') p++;
                } else {
                    skip_lf_ = true;
                }
            }
        }
        if (last) {
            skip_lf_ = false;
            if (has_pending_) {
                has_pending_ = false;
                std::string tail;
                tail.swap(pending_);
                if (!tail.empty() && !line((const uint8_t *)tail.data(), tail.size())) return false;
            }
        }
        return true;
    }

    int32_t node_of(const std::string &digits) const {
        if (digits.empty() || digits.size() > 10 || digits[0] == '0') return -1;
        int64_t v = 0;
        for (unsigned char c : digits) {
            if (c < '0' || c > '9') return -1;
            v = v * 10 + (c - '0');
        }
        if (v > INT32_MAX) return -1;
        const auto it = std::lower_bound(known.begin(), known.end(), (int32_t)v);
        return it != known.end() && *it == (int32_t)v ? (int32_t)(it - known.begin()) : -1;
    }

private:
    std::string pending_;
    bool has_pending_ = false, skip_lf_ = false;

    bool line(const uint8_t *p, size_t n) {
        const int64_t no = line_no++;
        if (n == 0 || p[0] == '#') {
            skipped++;
            return true;
        }
        size_t tab[21];  // tab[t]: the t-th tab of the line, tab[0]: one in front of the line
        size_t tabs = 0;
        for (size_t i = 0; i < n; i++)
            if (p[i] == '\t') {
                tabs++;
                if (tabs <= 20) tab[tabs] = i;
            }
        if (tabs < 19) {
            short_records++;
            return true;
        }
        counted++;
        if (tabs < 20) tab[20] = n;
        auto at = [&](int f) { return p + tab[f] + 1; };               // (field f lies between tab f and tab f + 1)
        auto len = [&](int f) { return tab[f + 1] - tab[f] - 1; };
        const int key = use_species ? 6 : 5;
        const int32_t node = node_of(asmsum_low_bytes(at(key), len(key)));
        if (node < 0) return true;
        if (!filter.empty() && !filter[(size_t)node]) return true;
        const int q = asmsum_quality(at(11), len(11), at(10), len(10));
        if (!(quality_mask >> q & 1)) return true;
        const bool is_ref = len(4) == 16 && memcmp(at(4), "reference genome", 16) == 0;
        if (reference_only && !is_ref) return true;
        if (len(19) == 0) {
            error = "a kept entry has an empty ftp path";
            return false;
        }
        AsmsumEntry e;
        e.node = node;
        e.quality = (uint8_t)q;
        e.is_ref = is_ref ? 1 : 0;
        e.line = no;
        e.taxid.assign((const char *)at(5), len(5));
        e.species.assign((const char *)at(6), len(6));
        e.ftp.assign((const char *)at(19), len(19));
        entries.push_back(std::move(e));
        return true;
    }
};

// the entries of a host-only handle and the cap of FastaFilesFromGenbankGoal: per node, a list longer than max_per_node > 0 is sorted
// stably, highest ordinal first, and cut from the front.  picked: entry numbers, nodes ascending, inside a node the list's order
struct AsmsumStore {
    std::vector<AsmsumEntry> entries;  // in input order
    std::vector<uint32_t> picked;
    int64_t nodes_with_entries = 0;

    void finish(int32_t max_per_node) {
        std::vector<uint32_t> seq(entries.size());
        for (size_t i = 0; i < seq.size(); i++) seq[i] = (uint32_t)i;
        std::stable_sort(seq.begin(), seq.end(), [this](uint32_t a, uint32_t b) { return entries[a].node < entries[b].node; });
        picked.clear();
        nodes_with_entries = 0;
        for (size_t i = 0; i < seq.size();) {
            size_t j = i;
            while (j < seq.size() && entries[seq[j]].node == entries[seq[i]].node) j++;
            nodes_with_entries++;
            size_t from = i;
            if (max_per_node > 0 && j - i > (size_t)max_per_node) {
                std::stable_sort(seq.begin() + (std::ptrdiff_t)i, seq.begin() + (std::ptrdiff_t)j,
                                 [this](uint32_t a, uint32_t b) { return entries[a].quality > entries[b].quality; });
                from = j - (size_t)max_per_node;
            }
            picked.insert(picked.end(), seq.begin() + (std::ptrdiff_t)from, seq.begin() + (std::ptrdiff_t)j);
            i = j;
        }
    }
};

}  // namespace gs_host
