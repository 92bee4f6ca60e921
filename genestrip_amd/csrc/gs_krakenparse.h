// gs_krakenparse.h -- the krakencount goal line by line, as the reference does it: KrakenResultProcessor.process
// (C/kraken/KrakenResultProcessor.java:74-179) under the listener of KrakenResCountGoal (C/goals/kraken/KrakenResCountGoal.java
// :133-157), over the lines of BufferedLineReader.nextLine (B/io/BufferedLineReader.java:160-182).  Pure host code without a
// device call or a thread: tests/native/krakenparse_sanitize.cpp runs it on its own.  It takes what the device refuses
// (gs_krakencount.hip), the unterminated tail of a file, and whole files under GS_HOST_FAST=0.
//
// Kept as the reference has it: NUL bytes are dropped, '\r' stays; a line is what nextLine returns less its last byte (the newline;
// of an unterminated tail: a byte of text) and the stream ENDS at the first line that is then empty; any ':' arms the token state
// for the rest of its line, the descriptor's included; a token whose first byte is 'A' is skipped, one whose tax id holds a
// non-digit too (the caught IllegalStateException); numbers are Java ints (they wrap); keys are strings ("007" is not "7");
// `reads` counts lines with at least one counted token, `kmers in matching reads` sees a line's first counted token only.
// Where the reference throws -- a non-digit in a count, the read size or the class -- feed() fails with the 1-based line.
// Deliberate difference: a line of more than 65 536 bytes with its newline makes the reference fail (array index); here it counts
// like any other and is reported (long_lines).
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace gs_host {

struct KrakenRow {
    int64_t reads = 0, kmers = 0, kimr = 0;
};

struct KrakenExact {
    std::map<std::string, KrakenRow> rows;  // (std::string orders bytes as DigitTrie.collect visits them: a prefix before its extensions)
    int64_t lines = 0, counted = 0, a_tokens = 0, long_lines = 0;
    int64_t line_no = 0;  // lines of the stream seen so far, wherever they were counted
    bool ended = false;   // the stream's first empty line, or its end, has been seen
    bool filtered = false;  // the caller selects rows by key afterwards (KrakenResCountGoal's taxIds != null)
    std::string error;    // why feed() failed

    // [p, p + n): whole lines; last: the stream ends behind them, and its final line need not be terminated.  false: the reference
    // throws on line line_no
    bool feed(const uint8_t *p, size_t n, bool last) {
        const uint8_t *end = p + n;
        while (p < end && !ended) {
            const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
            if (!nl && !last) break;  // (callers hand over whole lines)
            const uint8_t *stop = nl ? nl + 1 : end;
            line_.assign(p, stop);
            if (memchr(p, 0, (size_t)(stop - p))) {
                size_t w = 0;
                for (uint8_t c : line_)
                    if (c) line_[w++] = c;
                line_.resize(w);
            }
            p = stop;
            line_no++;
            if ((int64_t)line_.size() - 1 <= 0) {
                ended = true;
                break;
            }
            if (line_.size() > 65536) long_lines++;
            line_.pop_back();
            lines++;
            if (!line(line_.data(), line_.size())) return false;
        }
        if (last) ended = true;
        return true;
    }

    // a line counted elsewhere (the device): the next line sees its class field as that of the line before it
    void set_class_of(const uint8_t *s, size_t n) {
        const uint8_t *t1 = (const uint8_t *)memchr(s, '\t', n);
        const uint8_t *t2 = t1 ? (const uint8_t *)memchr(t1 + 1, '\t', (size_t)(s + n - t1 - 1)) : nullptr;
        const uint8_t *t3 = t2 ? (const uint8_t *)memchr(t2 + 1, '\t', (size_t)(s + n - t2 - 1)) : nullptr;
        if (!t3) return;
        cls_.assign((const char *)t2 + 1, (size_t)(t3 - t2 - 1));
        has_cls_ = true;
    }
    void forget_class() { has_cls_ = false; }  // a new stream

private:
    std::vector<uint8_t> line_;
    bool first_of_line_ = false;
    // the class of the last line that had one: the reference's classTaxid lives across lines, and is null before the first
    std::string cls_;
    bool has_cls_ = false;

    static bool digits(const uint8_t *s, size_t a, size_t b) {
        for (size_t i = a; i < b; i++)
            if (s[i] < '0' || s[i] > '9') return false;
        return true;
    }
    // ByteArrayUtil.byteArrayToInt
    bool to_int(const uint8_t *s, size_t a, size_t b, int32_t *out) {
        uint32_t v = 0;
        for (size_t i = a; i < b; i++) {
            if (s[i] < '0' || s[i] > '9') {
                error = "non-digit in a number";
                return false;
            }
            v = v * 10u + (uint32_t)(s[i] - '0');
        }
        *out = (int32_t)v;
        return true;
    }
    // the listener
    bool token(const std::string &taxid, int32_t n) {
        counted++;
        rows[taxid].kmers += n;
        if (!first_of_line_) return true;
        first_of_line_ = false;
        if (!has_cls_) {  // countingTrie.get(null, true) is null: the reference fails unless its tax id set filters the null away
            if (filtered) return true;
            error = "a token on a line without a class tax id";
            return false;
        }
        KrakenRow &r = rows[cls_];
        r.reads++;
        if (taxid == cls_) r.kimr += n;
        return true;
    }
    bool close(const uint8_t *s, size_t start_pos, size_t fr_start, size_t end) {
        int32_t n;
        if (!to_int(s, fr_start, end, &n)) return false;
        if (s[start_pos] == 'A') {
            a_tokens++;
            return true;
        }
        // (the count has parsed, so its ':' lies behind start_pos: a count that began in front of it would hold the delimiter)
        if (digits(s, start_pos, fr_start - 1)) return token(std::string((const char *)s + start_pos, fr_start - 1 - start_pos), n);
        return true;
    }
    bool line(const uint8_t *s, size_t n) {
        bool start = true, descriptor = false, class_id = false, read_size = false, fr = false;
        size_t start_pos = 0, fr_start = 0;
        first_of_line_ = true;
        for (size_t i = 0; i < n; i++) {
            if (s[i] == '\t') {
                if (start) {
                    start = false;
                    descriptor = true;
                } else if (descriptor) {
                    descriptor = false;
                    class_id = true;
                    start_pos = i + 1;
                } else if (class_id) {
                    class_id = false;
                    read_size = true;
                    if (!digits(s, start_pos, i)) {
                        error = "non-digit in the class tax id";
                        return false;
                    }
                    cls_.assign((const char *)s + start_pos, i - start_pos);
                    has_cls_ = true;
                    start_pos = i + 1;
                } else if (read_size) {
                    int32_t bps;
                    read_size = false;
                    if (!to_int(s, start_pos, i, &bps)) return false;
                    start_pos = i + 1;
                }
            } else if (s[i] == ':') {
                fr = true;
                fr_start = i + 1;
            } else if (fr && s[i] == ' ') {
                if (!close(s, start_pos, fr_start, i)) return false;
                start_pos = i + 1;
            }
        }
        if (start_pos < n && fr) return close(s, start_pos, fr_start, n);
        return true;
    }
};

}  // namespace gs_host
