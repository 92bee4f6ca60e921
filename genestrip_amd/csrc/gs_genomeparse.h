// gs_genomeparse.h -- a genome FASTA stream line by line, as the reference walks it: AbstractFastaReader.readFasta
// (C/fasta/AbstractFastaReader.java:97-130) over BufferedLineReader.nextLine (B/io/BufferedLineReader.java:160-182), with the bases
// of a data line as AbstractStoreFastaReader.dataLine (C/refseq/AbstractStoreFastaReader.java:87-114) puts them.  Pure host code
// without a device call or a thread: tests/native/genomeparse_sanitize.cpp runs it on its own.  It takes the chunks the device
// refuses (gs_genomes.hip: a NUL byte, a run of more than 64 '\r') and whole files under GS_HOST_FAST=0.
//
// Kept as the reference has it: NUL bytes are dropped before anything looks at the line; a line whose first byte is '>' ends the
// region in front of it and starts the next; data lines in front of the first header line are dropped; of a data line the whole
// trailing run of '\n' / '\r' goes (the while at :95 -- also a bare '\r' at the end of the stream), every other byte is a base; an
// empty line gives nothing.  Every region is kept here: which ones count is decided from the header lines afterwards.
// Deliberate difference: the reference throws when a line reaches fastaLineSizeBytes - 1; here the longest line is reported.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace gs_host {

struct GenomeRecords {
    std::vector<uint8_t> headers;      // the header lines from '>' up to but excluding the '\n', back to back
    std::vector<uint64_t> header_off;  // records + 1
    std::vector<uint8_t> seq;          // the bases of all records, back to back
    std::vector<uint64_t> off;         // records + 1, from 0
    int64_t max_line = 0;              // the longest line with its newline, NUL bytes not counted
    size_t consumed = 0;

    int64_t records() const { return (int64_t)off.size() - 1; }
};

// the bytes of [p, p + n) that the records which END there cover: all of them at the end of the stream, else up to the start of the
// last header line, without any header line up to behind the last newline
inline size_t genome_cut(const uint8_t *p, size_t n, bool last) {
    if (last) return n;
    for (size_t i = n; i-- > 0;)
        if (p[i] == '>' && (i == 0 || p[i - 1] == '\n')) return i;
    for (size_t i = n; i-- > 0;)
        if (p[i] == '\n') return i + 1;
    return 0;
}

// the records that end in [p, p + n) (genome_cut); `out` is replaced
inline void genome_parse(const uint8_t *p, size_t n, bool last, GenomeRecords *out) {
    out->headers.clear();
    out->seq.clear();
    out->header_off.assign(1, 0);
    out->off.assign(1, 0);
    out->max_line = 0;
    out->consumed = genome_cut(p, n, last);
    const uint8_t *end = p + out->consumed;
    std::vector<uint8_t> line;
    bool first = true;  // readFasta's flag: no region has been started
    while (p < end) {
        const uint8_t *nl = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
        const uint8_t *stop = nl ? nl + 1 : end;
        line.assign(p, stop);
        if (memchr(p, 0, (size_t)(stop - p))) {  // nextLine does not advance over a NUL byte
            size_t w = 0;
            for (uint8_t c : line)
                if (c) line[w++] = c;
            line.resize(w);
        }
        p = stop;
        const size_t size = line.size();
        if (size == 0) break;  // (NUL bytes alone behind the last newline: nextLine returns 0, the loop of readFasta ends)
        if ((int64_t)size > out->max_line) out->max_line = (int64_t)size;
        if (line[0] == '>') {
            if (!first) out->off.push_back(out->seq.size());  // endRegion
            first = false;
            out->headers.insert(out->headers.end(), line.begin(), line.end() - (line[size - 1] == '\n' ? 1 : 0));
            out->header_off.push_back(out->headers.size());
        } else if (!first) {
            size_t e = size;
            while (e > 0 && (line[e - 1] == '\n' || line[e - 1] == '\r')) e--;
            out->seq.insert(out->seq.end(), line.begin(), line.begin() + (std::ptrdiff_t)e);
        }
    }
    if (!first) out->off.push_back(out->seq.size());
}

}  // namespace gs_host
