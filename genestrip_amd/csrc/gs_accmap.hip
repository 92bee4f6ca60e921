// gs_accmap.hip -- lines of a RefSeq catalog to the accession map on the device (the accmapsize and accmap goals).
//
// The reference reads the catalog on one thread: AccessionFileProcessor.processCatalog (C/refseq/AccessionFileProcessor.java:96-131)
// finds the first five tabs of every line `taxid \t name \t accession \t categories \t status \t ...`, keeps an entry whose
// accession starts with a prefix of the selected sequence type and whose fourth and fifth fields hold one of the category and
// status strings, and AccessionMapGoal (C/goals/refseq/AccessionMapGoal.java:96-102) puts the accession of every kept entry whose
// tax id names a node of the tree.  AccessionMapImpl (C/refseq/AccessionMapImpl.java) sorts by length, then bytes.
//
// A chunk is taken here only if every line of it is inside a grammar on which the reference does the plain thing (gs_accmapparse.h
// restates what it does outside): five tabs and more on every line but "\n"; no NUL byte; no line above GS_AM_MAX_LINE bytes; and
// for an entry that passes the filter: a tax id of 1-9 digits without a leading zero, an accession of at most GS_AM_MAX_KEY bytes,
// all below 0x80.  Anything else refuses the chunk, which then writes nothing.
//
// A thread owns 16 bytes, a block GS_AM_TILE.  Newlines and tabs in front of every byte come from the block scan of gs_scan.h and
// gs_launch_scan_blocks over the per-tile sums.  The start of a byte's line and the tabs in front of that start both grow with the
// offset, so one max-scan of (line start << 32 | tabs in front of it) inside the block gives them; across tiles they come from
// the tile in front (tile_tail): a line that covers a whole tile is above GS_AM_MAX_LINE anyway.  The field of a byte is then
// (tabs in front of it) - (tabs in front of its line).
//   gs_am_tiles_kernel        per tile: newlines, tabs; its last newline and the tabs behind it                 1 read of the text
//   gs_am_scan_count_kernel   the grammar; the lane that owns a line's SECOND tab judges the entry: prefix (3 bytes), then -- only
//                             if that held -- the accession, category and status fields forwards and the tax id backwards, out of
//                             the LDS copy of the tile, 16 bytes in front of it and 32 behind, global memory beyond; per tile the
//                             entries it puts                                                                   1 read
//   gs_am_scan_write_kernel   (not launched for a refused chunk) the same decisions; slots at first_entry + the prefix of the puts;
//                             per-node region counts, equal nodes of a wave combined into one atomic            1 read
// In a real catalog most lines are protein records (WP_, XP_, NP_, YP_) that fail at the prefix: their judging lane reads 3 bytes.
//   gs_am_word_kernel, gs_am_permute_kernel, gs_am_dups_kernel   the finish: four stable rocPRIM sorts of (word, entry number)
//   gs_am_lookup_kernel       one lane per header line: first blank, prefix rule, probe key, lower bound in the sorted slots
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "gs_launch.h"
#include "gs_params.h"
#include "gs_scan.h"

#define AM_BLOCK GS_SCAN_BLOCK
static_assert(AM_BLOCK * 16 == GS_AM_TILE, "a thread owns 16 bytes of its tile");
#define AM_TEXT0 16                               // where the tile's first byte lies in its LDS copy
#define AM_TEXT_LDS (AM_TEXT0 + GS_AM_TILE + 32)  // 16 bytes in front of the tile, 32 behind it

__device__ __forceinline__ void am_masks(const uint4 &v, uint32_t &nlm, uint32_t &tabm, uint32_t &nulm) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    nlm = tabm = nulm = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        nlm |= (uint32_t)(b == '\n') << i;
        tabm |= (uint32_t)(b == '\t') << i;
        nulm |= (uint32_t)(b == 0) << i;
    }
}

__global__ __launch_bounds__(AM_BLOCK) void gs_am_tiles_kernel(GsAccmapParams P) {
    __shared__ uint32_t s_cnt[4];  // newlines, tabs, last newline + 1, tabs behind it
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = ((size_t)blockIdx.x * AM_BLOCK + threadIdx.x) * 16;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + base);
    uint32_t nlm, tabm, nulm;
    am_masks(v, nlm, tabm, nulm);
    // (bytes behind n_bytes are zero: neither newline nor tab)
    if (nlm) {
        atomicAdd(&s_cnt[0], (uint32_t)__popc(nlm));
        atomicMax(&s_cnt[2], threadIdx.x * 16u + (32u - (uint32_t)__clz(nlm)));
    }
    if (tabm) atomicAdd(&s_cnt[1], (uint32_t)__popc(tabm));
    __syncthreads();
    const uint32_t last = s_cnt[2];  // tile offset of the last newline + 1; 0: none
    uint32_t behind = 0;
    if (threadIdx.x * 16u + 16u > last) {
        const uint32_t from = last > threadIdx.x * 16u ? last - threadIdx.x * 16u : 0u;  // 0..15
        behind = (uint32_t)__popc(tabm >> from);
    }
    if (behind) atomicAdd(&s_cnt[3], behind);
    __syncthreads();
    if (threadIdx.x == 0) {
        P.tile_lt[blockIdx.x] = (u64)s_cnt[0] | (u64)s_cnt[1] << 32;
        P.tile_tail[blockIdx.x] = last | s_cnt[3] << 16;  // (both at most GS_AM_TILE)
    }
}

// exclusive prefix maximum of v over the block (every thread arrives); s_wave: AM_BLOCK / 64 words, free again behind one more barrier
__device__ __forceinline__ u64 am_block_max_scan(u64 v, u64 *s_wave) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 x = __shfl_up(inc, d);
        if (lane >= d && x > inc) inc = x;
    }
    u64 before = __shfl_up(inc, 1);
    if (lane == 0) before = 0;
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    for (int w = 0; w < wv; w++)
        if (s_wave[w] > before) before = s_wave[w];
    return before;
}

// the text as a judging lane sees it: the LDS copy where it reaches, global memory beyond; offsets are those of the chunk
struct AmText {
    const uint8_t *lds;  // lds[off - lo] for lo <= off < hi
    const uint8_t *glob;
    int64_t lo, hi, n_bytes;
    __device__ __forceinline__ uint32_t at(int64_t off) const {  // 0 <= off; behind the chunk: a newline
        if (off >= n_bytes) return '\n';
        return off >= lo && off < hi ? lds[off - lo] : glob[off];
    }
};

__device__ __forceinline__ void am_bad(const GsAccmapParams &P, uint32_t line) { atomicMin(&P.status[GS_AM_BAD_LINE], line); }

// does [a, b) hold one of the patterns [p0, p0 + n_pat) as a substring (ByteArrayUtil.indexOf over a String)
__device__ bool am_contains(const GsAccmapParams &P, const AmText &T, int64_t a, int64_t b, int p0, int n_pat) {
    for (int64_t i = a; i < b; i++) {
        const uint32_t c = T.at(i);
        for (int p = p0; p < p0 + n_pat; p++) {
            const int len = P.pat->len[p];
            if (P.pat->text[p][0] != c || i + len > b) continue;
            int j = 1;
            while (j < len && T.at(i + j) == P.pat->text[p][j]) j++;
            if (j == len) return true;
        }
    }
    return false;
}

struct AmEntry {
    int64_t acc;    // offset of the accession
    int32_t len;    // its bytes
    int32_t node;   // -1: passes, but its tax id names no node
};

// the entry of the line that starts at ls and has its second tab at pos2.  0: does not pass; 1: passes; 2: passes and is put
__device__ int am_judge(const GsAccmapParams &P, const AmText &T, int64_t ls, int64_t pos2, uint32_t line, AmEntry &e) {
    const uint32_t c0 = T.at(pos2 + 1), c1 = T.at(pos2 + 2), c2 = T.at(pos2 + 3);
    if (c2 != '_') return 0;
    const bool dna = c0 == 'A' ? c1 == 'C' : c0 == 'N' && (c1 == 'C' || c1 == 'G' || c1 == 'T' || c1 == 'W' || c1 == 'Z');
    const bool rna = (c0 == 'N' || c0 == 'X') && c1 == 'R';
    const bool mrna = (c0 == 'N' || c0 == 'X') && c1 == 'M';
    if (!((P.dna && dna) || (P.rna && rna) || (P.mrna && mrna))) return 0;
    // the third, fourth and fifth tab; a line without them, or above GS_AM_MAX_LINE, is refused by the lane at its end
    const int64_t limit = ls + GS_AM_MAX_LINE < P.n_bytes ? ls + GS_AM_MAX_LINE : P.n_bytes;
    int64_t pos[3];
    int found = 0;
    for (int64_t i = pos2 + 4; i < limit && found < 3; i++) {
        const uint32_t c = T.at(i);
        if (c == '\n') break;
        if (c == '\t') {
            if (found == 0) pos[0] = i;
            if (found == 1) pos[1] = i;
            if (found == 2) pos[2] = i;
            found++;
        }
    }
    if (found < 3) return 0;
    if (!am_contains(P, T, pos[0] + 1, pos[1], 0, P.n_cat)) return 0;
    if (!am_contains(P, T, pos[1] + 1, pos[2], GS_AM_MAX_PATTERNS, P.n_stat)) return 0;
    // it passes: the rest of the grammar
    e.acc = pos2 + 1;
    e.len = (int32_t)(pos[0] - pos2 - 1);
    e.node = -1;
    if (e.len > GS_AM_MAX_KEY) {
        am_bad(P, line);
        return 1;
    }
    for (int j = 3; j < e.len; j++)
        if (T.at(e.acc + j) >= 0x80u) am_bad(P, line);
    int64_t pos1 = pos2 - 1;  // the first tab: the only one between ls and pos2
    while (pos1 > ls && T.at(pos1) != '\t') pos1--;
    const int64_t digits = pos1 - ls;
    if (digits < 1 || digits > 9 || T.at(ls) == '0' || T.at(pos1) != '\t') {
        am_bad(P, line);
        return 1;
    }
    int32_t taxid = 0;
    for (int64_t i = ls; i < pos1; i++) {
        const uint32_t d = T.at(i) - '0';
        if (d > 9u) {
            am_bad(P, line);
            return 1;
        }
        taxid = taxid * 10 + (int32_t)d;
    }
    int32_t lo = 0, hi = P.n_nodes;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (P.known[mid] < taxid)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= P.n_nodes || P.known[lo] != taxid) return 1;
    e.node = lo;
    return 2;
}

// regions[node] += 1 for every lane with node >= 0; every lane of the wave arrives.  Equal nodes are combined first: the catalog
// lists the accessions of a species in runs
__device__ __forceinline__ void am_count_regions(int32_t *regions, int32_t node) {
    const int lane = threadIdx.x & 63;
    u64 todo = __ballot(node >= 0);
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int32_t its = __shfl(node, leader);
        const u64 same = __ballot(node == its);
        if (lane == leader) atomicAdd(&regions[its], (int32_t)__popcll(same));
        todo &= ~same;
    }
}

__device__ __forceinline__ void am_store_slot(const GsAccmapParams &P, const AmText &T, const AmEntry &e, int64_t slot) {
    uint32_t w[8] = {(uint32_t)e.len, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < GS_AM_MAX_KEY; j++) {
        const uint32_t b = j < e.len ? T.at(e.acc + j) : 0u;
        w[(j + 1) >> 2] |= b << (8 * ((j + 1) & 3));
    }
    uint4 *dst = reinterpret_cast<uint4 *>(P.keys + slot * 32);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    P.nodes[slot] = e.node;
}

template <bool WRITE>
__device__ __forceinline__ void am_scan_tile(const GsAccmapParams &P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[AM_TEXT_LDS];
    __shared__ u64 s_wave[3 * AM_BLOCK / 64];
    __shared__ uint32_t s_cnt[4];  // lines, passing, put, longest line
    const int64_t tile = blockIdx.x;
    const int64_t tile0 = tile * GS_AM_TILE;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + tile0 + threadIdx.x * 16);
    *reinterpret_cast<uint4 *>(s_text + AM_TEXT0 + threadIdx.x * 16) = v;
    if (threadIdx.x < 2)  // (the text's buffer ends 64 zero bytes behind its last tile)
        *reinterpret_cast<uint4 *>(s_text + AM_TEXT0 + GS_AM_TILE + threadIdx.x * 16) =
            *reinterpret_cast<const uint4 *>(P.text + tile0 + GS_AM_TILE + threadIdx.x * 16);
    if (threadIdx.x == 2)
        *reinterpret_cast<uint4 *>(s_text) = tile ? *reinterpret_cast<const uint4 *>(P.text + tile0 - 16) : make_uint4(0, 0, 0, 0);
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    AmText T;
    T.glob = P.text;
    T.lo = tile ? tile0 - AM_TEXT0 : 0;  // (nothing lies in front of the chunk)
    T.lds = s_text + AM_TEXT0 - (tile0 - T.lo);
    T.hi = tile0 + GS_AM_TILE + 32;
    T.n_bytes = P.n_bytes;

    uint32_t nlm, tabm, nulm;
    am_masks(v, nlm, tabm, nulm);
    const int64_t base = tile0 + threadIdx.x * 16;
    u64 total;
    const u64 tile_lt = P.tile_lt[tile];
    const u64 lt = gs_block_scan((u64)__popc(nlm) | (u64)__popc(tabm) << 32, s_wave, &total) + tile_lt;
    uint32_t L = (uint32_t)lt, g = (uint32_t)(lt >> 32);
    // where the line of my first byte starts, and the tabs in front of that start
    u64 mine = 0;
    if (nlm) {
        const int i = 31 - __clz(nlm);
        mine = (u64)(base + i + 1) << 32 | (u64)(g + (uint32_t)__popc(tabm & ((1u << i) - 1u)));
    }
    const u64 start = am_block_max_scan(mine, s_wave + AM_BLOCK / 64);
    int64_t ls = 0;
    uint32_t g0 = 0;
    if (start) {
        ls = (int64_t)(start >> 32);
        g0 = (uint32_t)start;
    } else if (tile) {  // (without a newline in the tile in front, the line is above GS_AM_MAX_LINE whatever ls says)
        const uint32_t tt = P.tile_tail[tile - 1];
        ls = tile0 - GS_AM_TILE + (tt & 0xffffu);
        g0 = (uint32_t)(tile_lt >> 32) - (tt >> 16);
    }

    const uint8_t *s = s_text + AM_TEXT0 + threadIdx.x * 16;
    uint32_t n_lines = 0, n_pass = 0, n_put = 0, longest = 0;
    AmEntry e0{0, 0, -1}, e1{0, 0, -1};
    for (int i = 0; i < 16 && base + i < P.n_bytes; i++) {
        const int64_t off = base + i;
        bool line_ends = false;
        if (nlm >> i & 1) {
            line_ends = true;
        } else {
            if (tabm >> i & 1) {
                if (g - g0 == 1) {
                    AmEntry e;
                    const int verdict = am_judge(P, T, ls, off, L, e);
                    n_pass += verdict >= 1;
                    if (verdict == 2) {
                        if (n_put == 0)
                            e0 = e;
                        else if (n_put == 1)
                            e1 = e;
                        else
                            am_bad(P, L);  // (three puts in 16 bytes: only on a line that is refused anyway)
                        n_put += n_put < 2;
                    }
                }
                g++;
            } else if (nulm >> i & 1) {
                am_bad(P, L);
            }
            if (off == P.n_bytes - 1) {  // the unterminated tail: BufferedLineReader hands it over with all its bytes if the stream ends
                if (!P.last || off - ls + 1 >= GS_AM_MAX_LINE) am_bad(P, L);
                line_ends = true;
            }
        }
        if (line_ends) {
            const uint32_t len = (uint32_t)(off - ls + 1);
            longest = len > longest ? len : longest;
            if (len > GS_AM_MAX_LINE)
                am_bad(P, L);
            else if (!(len == 1 && s[i] == '\n') && g - g0 < 5)
                am_bad(P, L);
            n_lines++;
            L++;
            ls = off + 1;
            g0 = g;
        }
    }
    if (!WRITE) {
        if (n_lines) atomicAdd(&s_cnt[0], n_lines);
        if (n_pass) atomicAdd(&s_cnt[1], n_pass);
        if (n_put) atomicAdd(&s_cnt[2], n_put);
        if (longest) atomicMax(&s_cnt[3], longest);
        __syncthreads();
        if (threadIdx.x == 0) {
            P.tile_put[tile] = s_cnt[2];
            if (s_cnt[0]) atomicAdd(&P.chunk[GS_AM_C_LINES], (u64)s_cnt[0]);
            if (s_cnt[1]) atomicAdd(&P.chunk[GS_AM_C_PASSING], (u64)s_cnt[1]);
            if (s_cnt[2]) atomicAdd(&P.chunk[GS_AM_C_PUT], (u64)s_cnt[2]);
            if (s_cnt[3]) atomicMax(&P.status[GS_AM_LONGEST], s_cnt[3]);
        }
    } else {
        const int64_t slot = P.first_entry + (int64_t)P.tile_put[tile] + (int64_t)gs_block_scan((u64)n_put, s_wave + 2 * AM_BLOCK / 64, &total);
        if (n_put >= 1 && slot < P.entry_cap) am_store_slot(P, T, e0, slot);
        if (n_put >= 2 && slot + 1 < P.entry_cap) am_store_slot(P, T, e1, slot + 1);
        am_count_regions(P.regions, n_put >= 1 ? e0.node : -1);
        am_count_regions(P.regions, n_put >= 2 ? e1.node : -1);
    }
}

__global__ __launch_bounds__(AM_BLOCK) void gs_am_scan_count_kernel(GsAccmapParams P) { am_scan_tile<false>(P); }
__global__ __launch_bounds__(AM_BLOCK) void gs_am_scan_write_kernel(GsAccmapParams P) { am_scan_tile<true>(P); }

// pass 1 of a chunk: P.status, P.chunk and the prefix of P.tile_put say what pass 2 would write.  P.n_bytes > 0
extern "C" hipError_t gs_launch_accmap_count(const GsAccmapParams *P, hipStream_t stream) {
    const unsigned n_tiles = (unsigned)P->n_tiles;
    hipLaunchKernelGGL(gs_am_tiles_kernel, dim3(n_tiles), dim3(AM_BLOCK), 0, stream, *P);
    hipError_t e = gs_launch_scan_blocks(P->tile_lt, P->n_tiles, P->scan_tot, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gs_am_scan_count_kernel, dim3(n_tiles), dim3(AM_BLOCK), 0, stream, *P);
    return gs_launch_scan_blocks(P->tile_put, P->n_tiles, P->scan_tot + 1, stream);
}

// pass 2, for a chunk that pass 1 did not refuse and whose entries have room
extern "C" hipError_t gs_launch_accmap_write(const GsAccmapParams *P, hipStream_t stream) {
    hipLaunchKernelGGL(gs_am_scan_write_kernel, dim3((unsigned)P->n_tiles), dim3(AM_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

// ---- the finish: a slot read as four big-endian words orders as the reference's compareBytes does (length, then bytes below 0x80)
__device__ __forceinline__ u64 am_word(const uint8_t *keys, int64_t entry, int w) {
    return __builtin_bswap64(reinterpret_cast<const u64 *>(keys)[entry * 4 + w]);
}

// word[i] = word w of entry seq[i] (seq == nullptr: of entry i, and seq_out[i] = i); *differs |= 1 if the words are not all equal
__global__ __launch_bounds__(256) void gs_am_word_kernel(const uint8_t *keys, const uint32_t *seq, int64_t n, int w, u64 *word, uint32_t *seq_out,
                                                         uint32_t *differs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 x = am_word(keys, seq ? seq[i] : i, w);
    word[i] = x;
    if (!seq) seq_out[i] = (uint32_t)i;
    if (x != am_word(keys, seq ? seq[0] : 0, w)) atomicOr(differs, 1u);
}

__global__ __launch_bounds__(256) void gs_am_permute_kernel(const uint8_t *keys, const int32_t *nodes, const uint32_t *seq, int64_t n, uint8_t *keys_out,
                                                            int32_t *nodes_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(keys + (size_t)seq[i] * 32);
    uint4 *dst = reinterpret_cast<uint4 *>(keys_out + (size_t)i * 32);
    dst[0] = src[0];
    dst[1] = src[1];
    nodes_out[i] = nodes[seq[i]];
}

// counts[0]: sorted entries equal to the one in front of them; counts[1]: those of them with another node
__global__ __launch_bounds__(256) void gs_am_dups_kernel(const uint8_t *keys, const int32_t *nodes, int64_t n, u64 *counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool dup = false, conflict = false;
    if (i >= 1 && i < n) {
        dup = true;
        for (int w = 0; w < 4; w++) dup = dup && am_word(keys, i, w) == am_word(keys, i - 1, w);
        conflict = dup && nodes[i] != nodes[i - 1];
    }
    const u64 d = __ballot(dup), c = __ballot(conflict);
    if ((threadIdx.x & 63) == 0) {
        if (d) atomicAdd(&counts[0], (u64)__popcll(d));
        if (c) atomicAdd(&counts[1], (u64)__popcll(c));
    }
}

extern "C" hipError_t gs_accmap_sort_bytes(int64_t n, size_t *tmp_bytes) {
    rocprim::double_buffer<u64> dk((u64 *)nullptr, (u64 *)nullptr);
    rocprim::double_buffer<uint32_t> dv((uint32_t *)nullptr, (uint32_t *)nullptr);
    *tmp_bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *tmp_bytes, dk, dv, (size_t)(n > 0 ? n : 1), 0, 64, (hipStream_t) nullptr);
}

extern "C" hipError_t gs_accmap_sort_entries(const uint8_t *keys, const int32_t *nodes, int64_t n, u64 *word, u64 *word_alt, uint32_t *seq, uint32_t *seq_alt,
                                       void *tmp, size_t tmp_bytes, uint32_t *flag, uint8_t *keys_out, int32_t *nodes_out, uint32_t **seq_out, u64 *counts,
                                       hipStream_t stream) {
    *seq_out = seq;
    hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(u64), stream);
    if (e != hipSuccess || n <= 0) return e;
    const unsigned grid = (unsigned)((n + 255) / 256);
    uint32_t *cur = nullptr, *alt = seq_alt;  // cur == nullptr: the identity, not written yet
    for (int w = 3; w >= 0; w--) {  // stable sorts from the last word to the first
        if ((e = hipMemsetAsync(flag, 0, sizeof(uint32_t), stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(gs_am_word_kernel, dim3(grid), dim3(256), 0, stream, keys, cur, n, w, word, seq, flag);
        uint32_t differs = 0;
        if ((e = hipMemcpyAsync(&differs, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        if (!cur) cur = seq;
        if (!differs) continue;  // a word that is equal over all entries orders nothing
        rocprim::double_buffer<u64> dk(word, word_alt);
        rocprim::double_buffer<uint32_t> dv(cur, alt);
        if ((e = rocprim::radix_sort_pairs(tmp, tmp_bytes, dk, dv, (size_t)n, 0, 64, stream)) != hipSuccess) return e;
        if (dv.current() != cur) {
            alt = cur;
            cur = dv.current();
        }
    }
    hipLaunchKernelGGL(gs_am_permute_kernel, dim3(grid), dim3(256), 0, stream, keys, nodes, cur, n, keys_out, nodes_out);
    hipLaunchKernelGGL(gs_am_dups_kernel, dim3(grid), dim3(256), 0, stream, keys_out, nodes_out, n, counts);
    *seq_out = cur;
    return hipGetLastError();
}

// ---- lookup: AbstractRefSeqFastaReader.updateNodeFromInfoLine over AccessionMapImpl.get
__global__ __launch_bounds__(256) void gs_am_lookup_kernel(const uint8_t *headers, const u64 *header_off, int64_t n, int complete_only, const uint8_t *keys,
                                                           const int32_t *nodes, int64_t n_entries, int32_t *node_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t *h = headers + header_off[i];
    const int64_t size = (int64_t)(header_off[i + 1] - header_off[i]);
    int64_t blank = 0;
    while (blank < size && h[blank] != ' ') blank++;
    int32_t node = -1;
    const int64_t len = blank - 1;  // the accession: [1, blank)
    bool search = blank < size && len >= 0 && len <= GS_AM_MAX_KEY;
    if (search && complete_only) {
        // AC_ NC_ NZ_ NM_ XM_ NR_ XR_ (a blank inside the three bytes matches none of them)
        const uint32_t c0 = len >= 3 ? h[1] : 0, c1 = len >= 3 ? h[2] : 0, c2 = len >= 3 ? h[3] : 0;
        search = c2 == '_' && ((c0 == 'A' && c1 == 'C') || (c0 == 'N' && (c1 == 'C' || c1 == 'Z' || c1 == 'M' || c1 == 'R')) ||
                               (c0 == 'X' && (c1 == 'M' || c1 == 'R')));
    }
    if (search) {
        u64 probe[4] = {(u64)len << 56, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < GS_AM_MAX_KEY; j++) {
            const u64 b = j < len ? h[1 + j] : 0;
            probe[(j + 1) >> 3] |= b << (8 * (7 - ((j + 1) & 7)));
        }
        int64_t lo = 0, hi = n_entries;  // the lowest entry that is not below the probe
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            bool below = false;
            for (int w = 0; w < 4; w++) {
                const u64 x = am_word(keys, mid, w);
                if (x != probe[w]) {
                    below = x < probe[w];
                    break;
                }
            }
            if (below)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo < n_entries && am_word(keys, lo, 0) == probe[0] && am_word(keys, lo, 1) == probe[1] && am_word(keys, lo, 2) == probe[2] &&
            am_word(keys, lo, 3) == probe[3])
            node = nodes[lo];
    }
    node_out[i] = node;
}

extern "C" hipError_t gs_launch_accmap_lookup(const uint8_t *headers, const u64 *header_off, int64_t n, int complete_only, const uint8_t *keys,
                                              const int32_t *nodes, int64_t n_entries, int32_t *node_out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_am_lookup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, headers, header_off, n, complete_only, keys, nodes,
                       n_entries, node_out);
    return hipGetLastError();
}
