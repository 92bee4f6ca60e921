// gs_chunk.h -- how the file loops of the host layer (gs_host.cpp) cut a stream of reader blocks into chunks of whole
// records.  Pure host code without a device call or a thread: tests/native/chunk_cut_check.cpp runs it on its own.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace gs_host {

// Where a FASTA chunk may end inside a block: header lines ('>' at a line start) are counted by memchr over the block ('>' is
// rare); the chunk ends in front of the block's last header line -- everything up to there is whole records --, at the end of
// the file behind the final newline.  cut < 0: no record boundary in this block.
struct FastaCut {
    int64_t headers = 0;      // header lines that start inside the block
    int64_t cut = -1;         // the chunk ends here (exclusive, offset in the block)
    int64_t cut_headers = 0;  // headers in front of `cut`
    int64_t tail_lines = 0;   // newlines at or behind `cut`
};

inline FastaCut fasta_cut(const uint8_t *blk, int64_t n, bool last, const std::vector<uint8_t> &carry) {
    FastaCut fc;
    const bool at_line_start = carry.empty() || carry.back() == '\n';
    int64_t last_hdr = -1;
    for (const uint8_t *p = blk, *end = blk + n; p < end;) {
        const uint8_t *q = (const uint8_t *)memchr(p, '>', (size_t)(end - p));
        if (!q) break;
        if (q == blk ? at_line_start : q[-1] == '\n') {
            fc.headers++;
            last_hdr = q - blk;
        }
        p = q + 1;
    }
    if (last && n > 0 && blk[n - 1] == '\n') {
        fc.cut = n;
        fc.cut_headers = fc.headers;
    } else if (last && n == 0 && !carry.empty() && carry.back() == '\n') {
        fc.cut = 0;
    } else if (last_hdr > 0 || (last_hdr == 0 && !carry.empty())) {
        fc.cut = last_hdr;
        fc.cut_headers = fc.headers - 1;
    }
    if (fc.cut >= 0)
        for (const uint8_t *p = blk + fc.cut, *end = blk + n; p < end;) {
            const uint8_t *q = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
            if (!q) break;
            fc.tail_lines++;
            p = q + 1;
        }
    return fc;
}

// One file's blocks, in order, into chunks of whole records.  A block lies behind `headroom` free bytes: what the last chunk
// left over (the carry) is copied in front of it, so that the chunk is one range and the reader's block goes to the device where
// it lies.  The chunk ends
//   FOUR_LINE  behind the last newline that closes a group of four lines,
//   FASTA      in front of the block's last header line (fasta_cut),
//   GENERAL    behind the block's last newline; the device then says how much of the chunk its records cover (commit),
//   LINES      behind the block's last newline: every line is a record of its own.
// A chunk the device took is committed -- only then does the carry move on; one it refused is not, and the general parser takes
// the file from file_off, the chunk's first byte.  The same offset serves when next() gives up (FALLBACK).
struct ChunkCutter {
    enum Mode { FOUR_LINE, FASTA, GENERAL, LINES };
    enum Cut {
        ABSORBED,  // nothing whole yet: the block went into the carry
        FALLBACK,  // a record longer than the headroom, or a FASTA chunk of 2^24 records or more: the general parser from file_off
        CHUNK      // [start, start + bytes): `lines` whole lines, `records` header lines (FASTA)
    };
    Mode mode = FOUR_LINE;
    std::vector<uint8_t> carry;  // what lies behind the last committed chunk
    int64_t carry_lines = 0, carry_headers = 0;
    int64_t file_off = 0;  // of the carry's first byte: where the next chunk starts in the (inflated) file
    uint8_t *start = nullptr;
    int64_t bytes = 0, lines = 0, records = 0;

    // block [blk, blk + n) with its newline count and the offsets of its last four newlines, last first (TextSlot); eof: the file's last
    Cut next(uint8_t *blk, int64_t n, int64_t newlines, const int64_t last4[4], bool eof, size_t headroom) {
        int64_t cut = -1, headers = 0;  // the chunk ends at blk + cut (exclusive)
        tail_lines_ = tail_headers_ = 0;
        if (mode == FOUR_LINE) {
            const int64_t total = carry_lines + newlines;
            tail_lines_ = total & 3;
            if (total >= 4) cut = last4[tail_lines_] + 1;  // the newline with that many newlines behind it ends the last whole record
        } else if (mode == FASTA) {
            const FastaCut fc = fasta_cut(blk, n, eof, carry);
            cut = fc.cut;
            headers = fc.headers;
            tail_lines_ = fc.tail_lines;
            tail_headers_ = fc.headers - fc.cut_headers;
        } else if (newlines > 0)
            cut = last4[0] + 1;
        if (cut < 0) {  // keep everything
            carry.insert(carry.end(), blk, blk + n);
            carry_lines += newlines;
            carry_headers += headers;
            return carry.size() > headroom && !eof ? FALLBACK : ABSORBED;
        }
        if (carry.size() > headroom) return FALLBACK;
        start = blk - carry.size();
        if (!carry.empty()) memcpy(start, carry.data(), carry.size());
        bytes = (int64_t)carry.size() + cut;
        lines = carry_lines + newlines - tail_lines_;
        records = carry_headers + headers - tail_headers_;
        rest_ = blk + cut;
        rest_end_ = blk + n;
        return mode == FASTA && records >= ((int64_t)1 << 24) ? FALLBACK : CHUNK;  // (more records than one chunk may hold)
    }
    // The device took the chunk: what lies behind the cut is the new carry.  The carry leaves the block here, so this comes before
    // the block is handed to a formatting thread or back to its reader.
    void commit() { commit(bytes, lines); }
    // GENERAL: its records cover used_bytes / used_lines of the chunk; what they do not cover is carried as well
    void commit(int64_t used_bytes, int64_t used_lines) {
        file_off += used_bytes;
        carry.assign(start + used_bytes, start + bytes);
        carry.insert(carry.end(), rest_, rest_end_);
        carry_lines = lines - used_lines + tail_lines_;
        carry_headers = tail_headers_;
    }

private:
    const uint8_t *rest_ = nullptr, *rest_end_ = nullptr;  // the block behind the cut
    int64_t tail_lines_ = 0, tail_headers_ = 0;            // newlines / header lines in it
};

}  // namespace gs_host
