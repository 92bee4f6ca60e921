// gs_accmapparse.h -- the accmapsize and accmap goals line by line, as the reference does them: AccessionFileProcessor.processCatalog
// (C/refseq/AccessionFileProcessor.java:96-131) under the handleEntry of AccessionMapGoal (C/goals/refseq/AccessionMapGoal.java:96-102),
// over the lines of BufferedLineReader.nextLine (B/io/BufferedLineReader.java:160-182); the order of AccessionMapImpl.compareBytes
// (C/refseq/AccessionMapImpl.java:154-165) and the search of AbstractRefSeqFastaReader.updateNodeFromInfoLine
// (C/refseq/AbstractRefSeqFastaReader.java:228-239).  Pure host code without a device call or a thread:
// tests/native/accmapparse_sanitize.cpp runs it on its own.  gs_host_accmap_files (gs_host.cpp) feeds it what the device refuses
// (gs_accmap.hip), the unterminated tail of a file, and whole files under GS_HOST_FAST=0.
//
// Kept as the reference has it:
//   * ONE line buffer of 2048 bytes lives across the lines of a stream, zeroed at its start.  A line is copied over its front; what
//     earlier lines left behind it stays.  With fewer than five tabs ByteArrayUtil.indexOf answers -1 and the next search starts
//     at 0 again, so fields overlap, and startsWith reads up to three bytes behind the line: stale ones.
//   * NUL bytes are dropped (each is written behind the line's end first, where the next byte of the line overwrites it).
//   * a line is what nextLine returns, its newline included; the last line of a stream may lack it.
//   * an entry passes on prefix, category and status alone and counts for the size; it is put only if its tax id field [0, pos1)
//     names a node: DigitTrie.getNode (C/util/DigitTrie.java:153-190) RETURNS NULL on a byte that is no digit -- it does not
//     throw -- and follows the digits as they stand, so "007" is not 7, and an empty field (or pos1 == -1) is the root, which holds
//     no node.  Such an entry counts and is not put.
//   * keys are bytes of any length here; the device's slots hold 31 (no accession of RefSeq comes near: they have 9 to 17 bytes),
//     a longer key is the caller's to refuse.
// Where the reference throws, feed() fails and names the 1-based line: a line that does not fit the buffer (2048 bytes without a
// newline among them: IllegalStateException), and a put with a negative length -- pos3 == -1 on a line of two tabs whose fields
// pass by overlap and whose first field names a node (Arrays.copyOfRange: IllegalArgumentException).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace gs_host {

struct AccmapEntry {
    std::string key;
    int32_t node;
};

struct AccmapExact {
    bool dna = false, rna = false, mrna = false;
    std::vector<std::string> categories, statuses;
    std::vector<int32_t> known;  // ascending, distinct, positive: a node is an index into it

    std::vector<AccmapEntry> entries;  // in input order
    int64_t passing = 0, lines = 0;
    int64_t line_no = 0;  // lines of the stream seen so far, wherever they were judged
    std::string error;    // why feed() failed

    AccmapExact() { begin_stream(); }
    void begin_stream() {  // processCatalog allocates its buffer anew
        memset(target_, 0, sizeof(target_));
        line_no = 0;
    }

    // [p, p + n): whole lines; last: the stream ends behind them and its final line need not be terminated.  false: the reference
    // throws on line line_no
    bool feed(const uint8_t *p, size_t n, bool last) {
        const uint8_t *end = p + n;
        while (p < end) {
            const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
            if (!nl && !last) break;  // (callers hand over whole lines)
            const uint8_t *stop = nl ? nl + 1 : end;
            int size = 0;
            if (!next_line(p, stop, &size)) {
                line_no++;
                error = "buffer is too small for a line in the accession catalog file";
                return false;
            }
            p = stop;
            if (size == 0) break;  // (NUL bytes alone at the end of the stream: nextLine returns 0)
            line_no++;
            lines++;
            if (!line(size)) return false;
        }
        return true;
    }

    // whole lines judged elsewhere (a chunk the device took: terminated, without NUL, none above the buffer) still leave their bytes in
    // the buffer.  Only a line longer than every line behind it shows: those are found from the end and copied oldest first.
    // (line_no is the caller's to advance.)
    void note_chunk(const uint8_t *p, size_t n) {
        std::vector<std::pair<const uint8_t *, size_t>> shows;
        size_t covered = 0;
        for (const uint8_t *end = p + n; end > p && covered < (size_t)MAX_LINE_SIZE;) {
            const uint8_t *nl = (const uint8_t *)memrchr(p, '\n', (size_t)(end - p) - 1);  // the newline in front of this line
            const uint8_t *start = nl ? nl + 1 : p;
            const size_t len = (size_t)(end - start);
            if (len > covered) {
                shows.push_back({start, len});
                covered = len;
            }
            end = start;
        }
        for (auto it = shows.rbegin(); it != shows.rend(); ++it) memcpy(target_, it->first, std::min(it->second, (size_t)MAX_LINE_SIZE));
    }

private:
    static const int MAX_LINE_SIZE = 2048;
    uint8_t target_[MAX_LINE_SIZE];

    // BufferedLineReader.nextLine over [p, stop); false: target.length + 1
    bool next_line(const uint8_t *p, const uint8_t *stop, int *size_out) {
        int size = 0;
        uint8_t c = 0xff;
        for (; p < stop; p++) {
            if (size == MAX_LINE_SIZE) return false;  // (c is no newline: the line would have ended)
            target_[size] = c = *p;
            if (c != 0) size++;
        }
        if (c != '\n' && size == MAX_LINE_SIZE) return false;
        *size_out = size;
        return true;
    }
    int index_of(int start, int end, uint8_t c) const {
        for (int i = start; i < end; i++)
            if (target_[i] == c) return i;
        return -1;
    }
    bool contains(int start, int end, const std::vector<std::string> &patterns) const {
        for (const std::string &s : patterns) {
            const int len = (int)s.size();
            for (int i = start; i <= end - len; i++)
                if (memcmp(target_ + i, s.data(), (size_t)len) == 0) return true;
        }
        return false;
    }
    bool starts_with(int start, const char *s) const {
        if (MAX_LINE_SIZE < start + 3) return false;
        return memcmp(target_ + start, s, 3) == 0;
    }
    bool any_prefix(int start, std::initializer_list<const char *> prefixes) const {
        for (const char *s : prefixes)
            if (starts_with(start, s)) return true;
        return false;
    }
    // DigitTrie.get over the canonical decimal strings of `known`
    int32_t node_of(int end) const {
        if (end < 1 || end > 10 || target_[0] == '0') return -1;
        int64_t v = 0;
        for (int i = 0; i < end; i++) {
            if (target_[i] < '0' || target_[i] > '9') return -1;
            v = v * 10 + (target_[i] - '0');
        }
        if (v > INT32_MAX) return -1;
        const auto it = std::lower_bound(known.begin(), known.end(), (int32_t)v);
        return it != known.end() && *it == (int32_t)v ? (int32_t)(it - known.begin()) : -1;
    }
    bool line(int size) {
        const int pos1 = index_of(0, size, '\t');
        const int pos2 = index_of(pos1 + 1, size, '\t');
        const int pos3 = index_of(pos2 + 1, size, '\t');
        const int pos4 = index_of(pos3 + 1, size, '\t');
        const int pos5 = index_of(pos4 + 1, size, '\t');
        if (!((dna && any_prefix(pos2 + 1, {"AC_", "NC_", "NG_", "NT_", "NW_", "NZ_"})) || (rna && any_prefix(pos2 + 1, {"NR_", "XR_"})) ||
              (mrna && any_prefix(pos2 + 1, {"NM_", "XM_"}))))
            return true;
        if (!contains(pos3 + 1, pos4, categories) || !contains(pos4 + 1, pos5, statuses)) return true;
        passing++;
        const int32_t node = node_of(pos1);
        if (node < 0) return true;
        if (pos3 < pos2 + 1) {
            error = "an entry without an accession field is put";
            return false;
        }
        entries.push_back({std::string((const char *)target_ + pos2 + 1, (size_t)(pos3 - pos2 - 1)), node});
        return true;
    }
};

// AccessionMapImpl: entries ordered by length, then (signed) bytes; among equal keys the first of the input stands in front, and
// that is the one a search answers with (the reference's answer depends on its quicksort there)
struct AccmapIndex {
    std::vector<AccmapEntry> sorted;
    static bool less(const std::string &a, const std::string &b) {
        if (a.size() != b.size()) return a.size() < b.size();
        for (size_t i = 0; i < a.size(); i++)
            if (a[i] != b[i]) return (int8_t)a[i] < (int8_t)b[i];
        return false;
    }
    void build(const std::vector<AccmapEntry> &entries) {
        sorted = entries;
        std::stable_sort(sorted.begin(), sorted.end(), [](const AccmapEntry &a, const AccmapEntry &b) { return less(a.key, b.key); });
    }
    // updateNodeFromInfoLine over one header line of `size` bytes
    int32_t lookup(const uint8_t *line, size_t size, bool complete_only) const {
        const uint8_t *blank = size ? (const uint8_t *)memchr(line, ' ', size) : nullptr;
        if (!blank || blank < line + 1) return -1;
        const std::string key((const char *)line + 1, (size_t)(blank - line - 1));
        if (complete_only) {
            bool ok = false;
            for (const char *s : {"AC_", "NC_", "NZ_", "NM_", "XM_", "NR_", "XR_"}) ok = ok || key.compare(0, 3, s) == 0;
            if (!ok) return -1;
        }
        const auto it = std::lower_bound(sorted.begin(), sorted.end(), key, [](const AccmapEntry &e, const std::string &k) { return less(e.key, k); });
        return it != sorted.end() && it->key == key ? it->node : -1;
    }
};

}  // namespace gs_host
