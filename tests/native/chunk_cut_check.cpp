// Stand-alone check of the block cutter of the host layer (genestrip_amd/csrc/gs_chunk.h; tests/test_host_cpu.py builds it with
// -fsanitize=address,undefined): texts go through ChunkCutter in blocks of 64, 100, 1000 and 4096 bytes with headroom == block, with
// `newlines` and `last4` computed the way TextReader::fill_newlines defines them.  Every block lives in an allocation of exactly
// headroom + n bytes, so a read or write outside of it is the sanitizer's to report.
//
// On records longer than the headroom: the cutter gives up when the CARRY outgrows the headroom, so a record of more than twice the
// headroom always ends in a fallback at its first byte, while one between one and two headrooms may also arrive whole (a carry of
// at most one headroom in front of a block that holds the rest).  Checked here: a fallback lies exactly at the first byte of a
// record that is longer than the headroom; the first record longer than twice the headroom -- or, if a fallback comes earlier, that
// one -- is where the chunks end; and no chunk ever holds a part of a record (every chunk is whole records by recount).
#include "../../genestrip_amd/csrc/gs_chunk.h"

#include <algorithm>
#include <cstdio>
#include <string>

using namespace gs_host;

static int fails = 0;
static int64_t seen[3][3];  // [mode][what next() returned]: every branch has to be reached
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            fails++;                             \
            fprintf(stderr, "FAIL %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);        \
            fprintf(stderr, "\n");               \
        }                                        \
    } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

struct Text {
    std::string name, bytes;
    std::vector<size_t> rec_start;  // first byte of every record (four-line and FASTA texts), + bytes.size()
    ChunkCutter::Mode mode;
};

// about forty four-line records of 40-300 bytes
static Text four_line(const char *name, const char *eol, bool final_newline) {
    Text t;
    t.name = name;
    t.mode = ChunkCutter::FOUR_LINE;
    for (int r = 0; r < 40; r++) {
        t.rec_start.push_back(t.bytes.size());
        const size_t L = 14 + rnd() % 131;  // 2 L + ~12 bytes per record
        std::string seq, qual;
        for (size_t i = 0; i < L; i++) {
            seq.push_back("ACGT"[rnd() & 3]);
            qual.push_back((char)('!' + rnd() % 40));
        }
        t.bytes += "@r" + std::to_string(r) + eol + seq + eol + "+" + eol + qual + eol;
    }
    if (!final_newline) t.bytes.pop_back();
    t.rec_start.push_back(t.bytes.size());
    return t;
}

// text in front of the first header, a '>' inside a data line, an empty record; pad_to > 0: short records behind them that make
// the text exactly that long (final newline included)
static Text fasta(const char *name, size_t pad_to) {
    Text t;
    t.name = name;
    t.mode = ChunkCutter::FASTA;
    t.bytes = "stray text\nin front\n";
    for (int r = 0; r < 30; r++) {
        t.rec_start.push_back(t.bytes.size());
        t.bytes += ">seq" + std::to_string(r) + " x\n";
        if (r == 7) continue;  // an empty record
        const int n_lines = 1 + (int)(rnd() % 4);
        for (int l = 0; l < n_lines; l++) {
            std::string line;
            const size_t L = 10 + rnd() % 70;
            for (size_t i = 0; i < L; i++) line.push_back("ACGT"[rnd() & 3]);
            if (r % 5 == 2 && l == 0) line[L / 2] = '>';  // not at a line start: no header
            t.bytes += line + "\n";
        }
    }
    while (pad_to > t.bytes.size()) {
        const size_t room = pad_to - t.bytes.size();
        t.rec_start.push_back(t.bytes.size());
        t.bytes += ">p\n" + std::string(room > 120 ? 50 : room - 4, 'A') + "\n";
    }
    t.rec_start.push_back(t.bytes.size());
    return t;
}

// sequence and quality over several lines; quality lines that start with '@'
static Text general_fastq() {
    Text t;
    t.name = "general FASTQ";
    t.mode = ChunkCutter::GENERAL;
    for (int r = 0; r < 40; r++) {
        const int n_lines = 1 + (int)(rnd() % 3);
        std::string seq, qual;
        for (int l = 0; l < n_lines; l++) {
            const size_t L = 5 + rnd() % 40;
            for (size_t i = 0; i < L; i++) seq.push_back("ACGT"[rnd() & 3]);
            seq.push_back('\n');
            qual += (r & 1) && l == 0 ? '@' : 'I';
            for (size_t i = 1; i < L; i++) qual.push_back((char)('!' + rnd() % 40));
            qual.push_back('\n');
        }
        t.bytes += "@g" + std::to_string(r) + "\n" + seq + "+\n" + qual;
    }
    return t;
}

static int64_t count(const uint8_t *p, int64_t n, char c) {
    int64_t k = 0;
    for (int64_t i = 0; i < n; i++) k += p[i] == (uint8_t)c;
    return k;
}

static void run(const Text &t, size_t block, bool expect_chunk_at_empty_eof = false) {
    const size_t headroom = block, len = t.bytes.size();
    ChunkCutter cut;
    cut.mode = t.mode;
    std::string got;   // the committed chunks in order
    std::string head;  // the carry behind the last commit: the next chunk starts with it
    int64_t fallback_off = -1, n_chunks = 0;
    bool chunk_at_empty_eof = false;
    for (size_t off = 0;; off += block) {
        const size_t n = off < len ? std::min(block, len - off) : 0;
        const bool eof = n < block;
        std::vector<uint8_t> buf(headroom + n);  // (exactly: the sanitizer sees every byte outside of it)
        uint8_t *blk = buf.data() + headroom;
        memcpy(blk, t.bytes.data() + off, n);
        const int64_t newlines = count(blk, (int64_t)n, '\n');
        int64_t last4[4];
        size_t end = n;
        for (int j = 0; j < 4; j++) {
            const void *q = end ? memrchr(blk, '\n', end) : nullptr;
            last4[j] = q ? (int64_t)((const uint8_t *)q - blk) : -1;
            end = q ? (size_t)((const uint8_t *)q - blk) : 0;
        }
        const int64_t chunk_off = cut.file_off;
        const ChunkCutter::Cut c = cut.next(blk, (int64_t)n, newlines, last4, eof, headroom);
        seen[t.mode][c]++;
        if (c == ChunkCutter::FALLBACK) {
            fallback_off = cut.file_off;
            CHECK(fallback_off == chunk_off, "%s/%zu: the fallback offset is not the refused chunk's start", t.name.c_str(), block);
            break;
        }
        if (c == ChunkCutter::CHUNK) {
            n_chunks++;
            chunk_at_empty_eof = chunk_at_empty_eof || n == 0;
            CHECK(cut.start >= buf.data() && cut.start + cut.bytes <= blk + n, "%s/%zu: chunk outside of its block", t.name.c_str(), block);
            CHECK((size_t)chunk_off == got.size(), "%s/%zu: chunk at %lld, %zu bytes committed", t.name.c_str(), block, (long long)chunk_off, got.size());
            CHECK((size_t)cut.bytes >= head.size() && memcmp(cut.start, head.data(), head.size()) == 0, "%s/%zu: what the last chunk left is not at the head of this one",
                  t.name.c_str(), block);
            CHECK(cut.lines == count(cut.start, cut.bytes, '\n'), "%s/%zu: %lld lines reported", t.name.c_str(), block, (long long)cut.lines);
            if (t.mode == ChunkCutter::FOUR_LINE)
                CHECK(cut.bytes > 0 && cut.start[cut.bytes - 1] == '\n' && cut.lines % 4 == 0 && cut.lines > 0, "%s/%zu: four-line chunk of %lld lines", t.name.c_str(),
                      block, (long long)cut.lines);
            if (t.mode == ChunkCutter::FASTA) {
                int64_t headers = 0;
                for (int64_t i = 0; i < cut.bytes; i++) headers += cut.start[i] == '>' && (i == 0 || cut.start[i - 1] == '\n');
                CHECK(cut.records == headers, "%s/%zu: %lld records reported, %lld header lines", t.name.c_str(), block, (long long)cut.records, (long long)headers);
                CHECK(n_chunks == 1 || (cut.bytes > 0 && cut.start[0] == '>'), "%s/%zu: a later FASTA chunk does not start with '>'", t.name.c_str(), block);
                CHECK(cut.bytes == 0 || cut.start[cut.bytes - 1] == '\n', "%s/%zu: FASTA chunk ends inside a line", t.name.c_str(), block);
            }
            if (t.mode == ChunkCutter::GENERAL) {
                // the device's part: its records cover all but the last two lines (a line boundary; nothing of a chunk of one or two lines)
                CHECK(cut.bytes > 0 && cut.start[cut.bytes - 1] == '\n', "%s/%zu: general chunk ends inside a line", t.name.c_str(), block);
                int64_t used = 0, used_lines = 0;
                for (int64_t i = 0; i < cut.bytes && used_lines < cut.lines - 2; i++)
                    if (cut.start[i] == '\n') {
                        used_lines++;
                        used = i + 1;
                    }
                CHECK(used < cut.bytes, "%s/%zu: the prefix is the whole chunk", t.name.c_str(), block);
                const std::string uncovered((const char *)cut.start + used, (size_t)(cut.bytes - used));
                got.append((const char *)cut.start, (size_t)used);
                cut.commit(used, used_lines);
                CHECK(cut.carry.size() >= uncovered.size() && memcmp(cut.carry.data(), uncovered.data(), uncovered.size()) == 0,
                      "%s/%zu: the uncovered lines are not at the head of the carry", t.name.c_str(), block);
                CHECK(cut.carry_lines == cut.lines - used_lines, "%s/%zu: %lld lines carried", t.name.c_str(), block, (long long)cut.carry_lines);
            } else {
                got.append((const char *)cut.start, (size_t)cut.bytes);
                cut.commit();
            }
            head.assign((const char *)cut.carry.data(), cut.carry.size());
            CHECK((size_t)cut.file_off == got.size(), "%s/%zu: file_off %lld after %zu bytes", t.name.c_str(), block, (long long)cut.file_off, got.size());
        }
        CHECK(cut.carry_lines == count(cut.carry.data(), (int64_t)cut.carry.size(), '\n'), "%s/%zu: carry_lines %lld", t.name.c_str(), block, (long long)cut.carry_lines);
        CHECK(cut.file_off + (int64_t)cut.carry.size() == (int64_t)(off + n), "%s/%zu: the carry does not end where the block does", t.name.c_str(), block);
        if (eof) break;
    }
    // the committed chunks, then the final carry or the bytes from the fallback offset on, are the input
    std::string all = got;
    if (fallback_off >= 0) {
        CHECK((size_t)fallback_off == got.size(), "%s/%zu: fallback at %lld behind %zu committed bytes", t.name.c_str(), block, (long long)fallback_off, got.size());
        all += t.bytes.substr((size_t)fallback_off);
    } else
        all.append((const char *)cut.carry.data(), cut.carry.size());
    CHECK(all == t.bytes, "%s/%zu: chunks + rest differ from the input (%zu against %zu bytes)", t.name.c_str(), block, all.size(), t.bytes.size());
    if (expect_chunk_at_empty_eof) CHECK(chunk_at_empty_eof, "%s/%zu: no chunk from the empty last block", t.name.c_str(), block);
    if (t.mode == ChunkCutter::GENERAL) {
        CHECK(fallback_off <= 0 || t.bytes[(size_t)fallback_off - 1] == '\n', "%s/%zu: fallback inside a line", t.name.c_str(), block);
        return;
    }
    // records longer than the headroom
    size_t first_2x = t.rec_start.size() - 1;  // index of the first record of more than two headrooms
    for (size_t r = 0; r + 1 < t.rec_start.size(); r++)
        if (t.rec_start[r + 1] - t.rec_start[r] > 2 * headroom) {
            first_2x = r;
            break;
        }
    if (fallback_off >= 0) {
        size_t r = 0;
        while (r + 1 < t.rec_start.size() && t.rec_start[r] != (size_t)fallback_off) r++;
        CHECK(r + 1 < t.rec_start.size(), "%s/%zu: fallback at %lld, not a record's first byte", t.name.c_str(), block, (long long)fallback_off);
        if (r + 1 < t.rec_start.size())
            CHECK(t.rec_start[r + 1] - t.rec_start[r] > headroom, "%s/%zu: fallback at record %zu of %zu bytes", t.name.c_str(), block, r, t.rec_start[r + 1] - t.rec_start[r]);
        CHECK(r <= first_2x, "%s/%zu: a chunk took record %zu of more than two headrooms", t.name.c_str(), block, first_2x);
    } else
        CHECK(first_2x + 1 == t.rec_start.size(), "%s/%zu: no fallback at record %zu of more than two headrooms", t.name.c_str(), block, first_2x);
}

int main() {
    const Text texts[] = {four_line("four-line", "\n", true), four_line("four-line CRLF", "\r\n", true), four_line("four-line, no final newline", "\n", false),
                          fasta("FASTA", 0), general_fastq()};
    for (const Text &t : texts)
        for (size_t block : {64, 100, 1000, 4096}) run(t, block);
    // without a final newline the last block is absorbed: what it holds is the parser's
    for (Text t : {fasta("FASTA, no final newline", 0), general_fastq()}) {
        t.bytes.pop_back();
        if (!t.rec_start.empty()) t.rec_start.back()--;
        for (size_t block : {64, 100, 1000, 4096}) run(t, block);
    }
    // ... and so is a last block that is the middle of a line: the texts cut off one byte into a block of 1000
    for (Text t : {fasta("FASTA, cut off", 0), general_fastq()}) {
        size_t base = t.bytes.size() / 1000 * 1000;
        while (t.bytes[base] == '\n' || t.bytes[base - 1] == '\n') base -= 1000;
        t.bytes.resize(base + 1);
        while (!t.rec_start.empty() && t.rec_start.back() >= t.bytes.size()) t.rec_start.pop_back();
        t.rec_start.push_back(t.bytes.size());
        run(t, 1000);
    }
    // an end-of-file block with n == 0 behind a carry that ends in '\n': a FASTA text of exactly six blocks
    run(fasta("FASTA of whole blocks", 6000), 1000, true);
    for (int m = 0; m < 3; m++) {
        printf("mode %d: %lld blocks absorbed, %lld fallbacks, %lld chunks\n", m, (long long)seen[m][ChunkCutter::ABSORBED], (long long)seen[m][ChunkCutter::FALLBACK],
               (long long)seen[m][ChunkCutter::CHUNK]);
        for (int c = 0; c < 3; c++) CHECK(seen[m][c] > 0, "mode %d never gave result %d", m, c);
    }
    printf("fails %d\n", fails);
    return fails ? 1 : 0;
}
