// gs_indexfile.h -- the native index file of gs_bloom_save / gs_bloom_load (include/gsgpu.h): header | hash factors | words.
// Host code only and free of HIP, so that the reader and its checks also build as a plain C++ program
// (tests/native/indexfile_sanitize.cpp runs them under the address and undefined-behaviour sanitizers).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/types.h>

#include <string>
#include <vector>

#include "../../include/gsgpu.h"
#include "gs_checksum.h"

struct GsIndexFileHeader {
    char magic[8];  // "GSINDEX1"
    int32_t kind, k, n_hashes, pad;
    int64_t bits, n_words, expected_insertions, n_inserted;
    double fpp;
    uint64_t checksum;  // StoreChecksum over factors | words
};
static_assert(sizeof(GsIndexFileHeader) == 72, "the index file header is 72 bytes");

enum { GS_INDEXFILE_OK = 0, GS_INDEXFILE_DEFECT = 1, GS_INDEXFILE_IO = 2 };

// what is wrong with a header (nullptr: nothing): every field the loader or a kernel sizes or indexes with
static inline const char *gs_index_header_defect(const GsIndexFileHeader &h) {
    if (memcmp(h.magic, "GSINDEX1", 8) != 0) return "not a gsgpu index file (or one of another layout version)";
    if (h.kind < GS_BLOOM_XOR || h.kind > GS_BLOOM_BLOCKED) return "unknown filter kind";
    if (h.k < 0 || h.k > 31) return "k out of range";
    if (h.n_hashes < 1 || h.n_hashes > 64) return "n_hashes outside [1, 64]";
    if (h.kind == GS_BLOOM_BLOCKED) {
        if (h.n_hashes != 1) return "a blocked filter has one seed";
        if (h.bits < 1 || h.bits > ((int64_t)1 << 40)) return "bucket count out of range";
        if (h.n_words != h.bits + 17) return "n_words does not match the bucket count";
    } else {
        if (h.bits < 1 || h.bits > ((int64_t)1 << 37)) return "bit count out of range";
        if (h.n_words != (h.bits + 63) / 64) return "n_words does not match the bit count";
    }
    return nullptr;
}

static inline uint64_t gs_index_checksum(const std::vector<int64_t> &factors, const std::vector<unsigned long long> &words) {
    StoreChecksum cs;
    cs.add(factors.data(), factors.size() * sizeof(int64_t));
    cs.add(words.data(), words.size() * sizeof(unsigned long long));
    return cs.value();
}

// The whole file, checked: header fields, the exact file length, then the payload and its checksum.  GS_INDEXFILE_DEFECT: the
// file is not a sound index file; GS_INDEXFILE_IO: it cannot be opened or read.  `why` names the path and the reason.
static inline int gs_index_file_read(const char *path, GsIndexFileHeader &h, std::vector<int64_t> &factors, std::vector<unsigned long long> &words,
                                     std::string &why) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        why = std::string("cannot open ") + path;
        return GS_INDEXFILE_IO;
    }
    h = GsIndexFileHeader{};
    const char *defect = fread(&h, sizeof(h), 1, f) == 1 ? gs_index_header_defect(h) : "truncated header";
    if (!defect) {  // the payload the header announces must be exactly what the file holds
        const uint64_t want = (uint64_t)sizeof(h) + 8 * ((uint64_t)h.n_hashes + (uint64_t)h.n_words);
        const off_t size = fseeko(f, 0, SEEK_END) == 0 ? ftello(f) : (off_t)-1;
        if (size < 0) {
            fclose(f);
            why = std::string("cannot read ") + path;
            return GS_INDEXFILE_IO;
        }
        if ((uint64_t)size != want) defect = (uint64_t)size < want ? "file shorter than its header announces (truncated)" : "file longer than its header announces";
    }
    if (defect) {
        fclose(f);
        why = std::string(path) + ": " + defect;
        return GS_INDEXFILE_DEFECT;
    }
    factors.assign((size_t)h.n_hashes, 0);
    words.assign((size_t)h.n_words, 0);
    const bool got = fseeko(f, (off_t)sizeof(h), SEEK_SET) == 0 && fread(factors.data(), sizeof(int64_t), factors.size(), f) == factors.size() &&
                     fread(words.data(), sizeof(unsigned long long), words.size(), f) == words.size();
    fclose(f);
    if (!got) {
        why = std::string("cannot read ") + path;
        return GS_INDEXFILE_IO;
    }
    if (gs_index_checksum(factors, words) != h.checksum) {
        why = std::string(path) + ": payload checksum mismatch (damaged file)";
        return GS_INDEXFILE_DEFECT;
    }
    return GS_INDEXFILE_OK;
}
