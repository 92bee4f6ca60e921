// The reader of the native index file (genestrip_amd/csrc/gs_indexfile.h: header checks, file length, payload, checksum) as a
// program of its own, for a sanitizer build (tests/test_index_cpu.py compiles it with -fsanitize=address,undefined and runs it on
// sound and damaged files).  Prints one line per path: "<verdict> <n_hashes> <n_words> <message>" with verdict 0 = sound,
// 1 = defect, 2 = cannot be read -- what gs_bloom_load turns into GS_OK (or a device error), GS_E_INVALID and GS_E_IO.
#include <stdio.h>

#include <string>
#include <vector>

#include "../../genestrip_amd/csrc/gs_indexfile.h"

static volatile unsigned long long sink;

int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) {
        GsIndexFileHeader h;
        std::vector<int64_t> factors;
        std::vector<unsigned long long> words;
        std::string why;
        const int verdict = gs_index_file_read(argv[i], h, factors, words, why);
        unsigned long long touched = 0;  // every word the loader would upload is readable
        for (unsigned long long w : words) touched ^= w;
        for (int64_t f : factors) touched ^= (unsigned long long)f;
        sink = touched;
        printf("%d %zu %zu %s\n", verdict, factors.size(), words.size(), why.c_str());
    }
    return 0;
}
