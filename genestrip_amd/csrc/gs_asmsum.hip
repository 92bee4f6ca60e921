// gs_asmsum.hip -- lines of a Genbank assembly summary to the picks per tree node on the device (the fastasgenbank goal).
//
// The reference reads assembly_summary_genbank.txt on one thread through Commons CSV: AssemblySummaryReader.getRelevantEntries
// (C/genbank/AssemblySummaryReader.java:104-144) keeps an entry of 20 fields and more whose tax id (or species tax id) names a node
// of the tree inside the filter, whose quality (assembly level and version status) is allowed and which, if asked for, is a
// reference genome; FastaFilesFromGenbankGoal (C/goals/genbank/FastaFilesFromGenbankGoal.java:101-150) then keeps the best
// max_per_node of a node.  gs_asmsumparse.h restates the rules record by record.
//
// A chunk is taken here only if every line of it is inside this grammar:
//   * no '\r' anywhere (NCBI writes LF; the CR rules stay host logic);
//   * no line above GS_AS_MAX_LINE = 4096 bytes with its newline (real lines reach 700); an unterminated last line only if the
//     stream ends with the chunk;
//   * no byte from 0x80 on inside the KEY field (tax id, or species tax id) of a record of 20 fields and more -- everywhere else
//     such bytes are data;
//   * no kept entry with an empty ftp field (the reference throws there).
// Anything else refuses the chunk, which then writes nothing.  A key that is not 1-9 digits without a leading zero names no node.
//
// A thread owns 16 bytes, a block GS_AS_TILE.  Newlines and tabs in front of every byte come from the block scan of gs_scan.h and
// gs_launch_scan_blocks over the per-tile sums, the start of a byte's line and the tabs in front of it from one max-scan of
// (line start << 32 | tabs in front of it), as in gs_accmap.hip.  A line here has hundreds of bytes and the six fields that
// decide are spread over it, so NO LANE WALKS A LINE:
//   gs_as_tiles_kernel   per tile: newlines, tabs; its last newline and the tabs behind it                       1 read of the text
//   gs_as_slots_kernel   the lanes that own tabs number 4 5 6 7 10 11 12 19 20 of a line store their offsets into the line's slot
//                        (32 bytes, indexed by the line's number in the chunk), the lane at its end the line's start, tabs and
//                        length; a lane with a byte from 0x80 on in the key field marks the line; CR and long lines refuse    1 read
//   gs_as_judge_kernel   one lane per LINE: the slot, then two constant compares, the quality table, the key parsed and searched in
//                        known_taxids, the filter flag -> the line's verdict; per block of lines kept entries and pool bytes
//   gs_as_write_kernel   (not launched for a refused chunk) entries in input order at first_entry + the prefix of the kept
//   gs_as_gather_kernel  16 lanes per entry copy its three strings into the pool
//   gs_as_node_count_kernel, gs_as_pick_kernel, gs_as_key_kernel, gs_as_place_kernel   the cap: entries per node, one stable rocPRIM
//                        radix sort of (node, capped(node) ? 10 - ordinal : 0) with the entry number as value -- nodes that are not
//                        cut keep input order --, the rank inside the node from the prefix of the counts, the survivors
//                        rank >= count - max placed at the prefix of the picks
//   gs_as_pick_len_kernel, gs_as_pick_gather_kernel   the picked entries and their strings, compacted for the fetch
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gs_launch.h"
#include "gs_params.h"
#include "gs_scan.h"

#define AS_BLOCK GS_SCAN_BLOCK
static_assert(AS_BLOCK * 16 == GS_AS_TILE, "a thread owns 16 bytes of its tile");
static_assert(GS_AS_MAX_LINE <= GS_AS_TILE, "a line that covers a whole tile is above GS_AS_MAX_LINE");
static_assert(sizeof(GsAsmEntry) == 40, "an entry has 40 bytes");
static_assert(GS_AS_LINE_BLOCK == AS_BLOCK, "a judging block is a scan block");

__device__ __forceinline__ void as_masks(const uint4 &v, uint32_t &nlm, uint32_t &tabm, uint32_t &crm, uint32_t &him) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    nlm = tabm = crm = him = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        nlm |= (uint32_t)(b == '\n') << i;
        tabm |= (uint32_t)(b == '\t') << i;
        crm |= (uint32_t)(b == '\r') << i;
        him |= (uint32_t)(b >= 0x80u) << i;
    }
}

__global__ __launch_bounds__(AS_BLOCK) void gs_as_tiles_kernel(GsAsmsumParams P) {
    __shared__ uint32_t s_cnt[4];  // newlines, tabs, last newline + 1, tabs behind it
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = ((size_t)blockIdx.x * AS_BLOCK + threadIdx.x) * 16;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + base);
    uint32_t nlm, tabm, crm, him;
    as_masks(v, nlm, tabm, crm, him);
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
        P.tile_tail[blockIdx.x] = last | s_cnt[3] << 16;  // (both at most GS_AS_TILE)
    }
}

// exclusive prefix maximum of v over the block (every thread arrives); s_wave: AS_BLOCK / 64 words
__device__ __forceinline__ u64 as_block_max_scan(u64 v, u64 *s_wave) {
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

__device__ __forceinline__ void as_bad(const GsAsmsumParams &P, uint32_t line) { atomicMin(&P.status[GS_AS_BAD_LINE], line); }

// where the t-th tab of a line goes in its slot; -1: nowhere
__device__ __forceinline__ int as_tab_word(uint32_t t) {
    if (t >= 4 && t <= 7) return (int)t - 4;
    if (t >= 10 && t <= 12) return (int)t - 6;
    if (t == 19 || t == 20) return (int)t - 12;
    return -1;
}

__device__ __forceinline__ uint16_t as_u16(int64_t x) { return (uint16_t)(x > 0xffff ? 0xffff : x); }

__global__ __launch_bounds__(AS_BLOCK) void gs_as_slots_kernel(GsAsmsumParams P) {
    __shared__ u64 s_wave[2 * AS_BLOCK / 64];
    __shared__ uint32_t s_longest;
    const int64_t tile = blockIdx.x;
    const int64_t tile0 = tile * GS_AS_TILE;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + tile0 + threadIdx.x * 16);
    if (threadIdx.x == 0) s_longest = 0;
    uint32_t nlm, tabm, crm, him;
    as_masks(v, nlm, tabm, crm, him);
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
    const u64 start = as_block_max_scan(mine, s_wave + AS_BLOCK / 64);
    int64_t ls = 0;
    uint32_t g0 = 0;
    if (start) {
        ls = (int64_t)(start >> 32);
        g0 = (uint32_t)start;
    } else if (tile) {  // (without a newline in the tile in front, the line is above GS_AS_MAX_LINE whatever ls says)
        const uint32_t tt = P.tile_tail[tile - 1];
        ls = tile0 - GS_AS_TILE + (tt & 0xffffu);
        g0 = (uint32_t)(tile_lt >> 32) - (tt >> 16);
    }

    uint32_t longest = 0;
    for (int i = 0; i < 16 && base + i < P.n_bytes; i++) {
        const int64_t off = base + i;
        bool line_ends = false;
        int64_t len = 0, len_nl = 0;  // the line's bytes without and with its newline
        if (nlm >> i & 1) {
            line_ends = true;
            len = off - ls;
            len_nl = len + 1;
        } else {
            if (crm >> i & 1) as_bad(P, L);
            if (tabm >> i & 1) {
                const int w = as_tab_word(g - g0 + 1);
                if (w >= 0 && (int64_t)L < P.n_lines) P.slots[(size_t)L * GS_AS_SLOT + GS_AS_S_TAB + w] = as_u16(off - ls);
                g++;
            } else if ((him >> i & 1) && (int32_t)(g - g0) == P.key_field && (int64_t)L < P.n_lines) {
                P.high[L] = 1;
            }
            if (off == P.n_bytes - 1) {  // the unterminated tail: a record only if the stream ends here
                if (!P.last) as_bad(P, L);
                line_ends = true;
                len = len_nl = off - ls + 1;
            }
        }
        if (line_ends) {
            longest = len_nl > (int64_t)longest ? (uint32_t)len_nl : longest;
            if (len_nl > GS_AS_MAX_LINE) as_bad(P, L);
            if ((int64_t)L < P.n_lines) {
                uint16_t *slot = P.slots + (size_t)L * GS_AS_SLOT;
                *reinterpret_cast<uint32_t *>(slot + GS_AS_S_START) = (uint32_t)ls;
                slot[GS_AS_S_TABS] = as_u16(g - g0);
                slot[GS_AS_S_LEN] = as_u16(len);
            }
            L++;
            ls = off + 1;
            g0 = g;
        }
    }
    if (longest) atomicMax(&s_longest, longest);
    __syncthreads();
    if (threadIdx.x == 0 && s_longest) atomicMax(&P.status[GS_AS_LONGEST], s_longest);
}

// what a judging lane knows of its line
struct AsLine {
    int64_t ls;        // its first byte in the chunk
    int32_t len;       // its bytes without the terminator; <= GS_AS_MAX_LINE
    int32_t tabs;
    int32_t tab[9];    // tabs number 4 5 6 7 10 11 12 19 20 as offsets from ls, none beyond len (the terminator stands for tab 20)
};

// false: no record to judge here (a line above the limit: the chunk is refused already)
__device__ __forceinline__ bool as_read_slot(const GsAsmsumParams &P, int64_t L, AsLine &ln) {
    const uint4 *sp = reinterpret_cast<const uint4 *>(P.slots + (size_t)L * GS_AS_SLOT);
    const uint4 a = sp[0], b = sp[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    ln.ls = (int64_t)w[0];
    ln.tabs = (int32_t)(w[1] & 0xffffu);
    ln.len = (int32_t)(w[1] >> 16);
    if (ln.len > GS_AS_MAX_LINE || ln.ls + ln.len > P.n_bytes) return false;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int h = GS_AS_S_TAB + k;
        const int32_t t = (int32_t)((w[h >> 1] >> (16 * (h & 1))) & 0xffffu);
        ln.tab[k] = t < ln.len ? t : ln.len;
    }
    if (ln.tabs < 20) ln.tab[8] = ln.len;
    return true;
}

__device__ __forceinline__ bool as_equals(const uint8_t *p, int32_t n, const char *lit, int32_t n_lit) {
    if (n != n_lit) return false;
    bool eq = true;
#pragma nounroll
    for (int32_t i = 0; i < n_lit; i++) eq = eq && p[i] == (uint8_t)lit[i];  // (not unrolled: the literals stay in memory, not in scalar registers)
    return eq;
}

// the verdict of line L (0: nothing kept) and the bytes of its three strings
__device__ u64 as_judge(const GsAsmsumParams &P, int64_t L, const AsLine &ln, uint32_t *bytes) {
    const uint8_t *t = P.text + ln.ls;
    // fields 4 5 6 10 11 19 lie between tabs (4,5) (5,6) (6,7) (10,11) (11,12) (19,20): slot words 0 1 2 3 | 4 5 6 | 7 8
    const int ka = P.key_field == 5 ? 1 : 2;
    const int32_t k0 = ln.tab[ka] + 1, klen = ln.tab[ka + 1] - k0;
    if (klen < 1 || klen > 9 || t[k0] == '0') return 0;
    int32_t taxid = 0;
    for (int32_t i = 0; i < klen; i++) {
        const uint32_t d = (uint32_t)t[k0 + i] - '0';
        if (d > 9u) return 0;
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
    if (lo >= P.n_nodes || P.known[lo] != taxid) return 0;
    if (P.filter && !P.filter[lo]) return 0;
    const bool latest = as_equals(t + ln.tab[4] + 1, ln.tab[5] - ln.tab[4] - 1, "latest", 6);
    const uint8_t *lv = t + ln.tab[5] + 1;
    const int32_t n_lv = ln.tab[6] - ln.tab[5] - 1;
    uint32_t q = latest ? 9 : 10;
    if (as_equals(lv, n_lv, "Complete Genome", 15)) q = latest ? 1 : 2;
    else if (as_equals(lv, n_lv, "Chromosome", 10)) q = latest ? 3 : 4;
    else if (as_equals(lv, n_lv, "Scaffold", 8)) q = latest ? 5 : 6;
    else if (as_equals(lv, n_lv, "Contig", 6)) q = latest ? 7 : 8;
    if (!(P.quality_mask >> q & 1)) return 0;
    const bool is_ref = as_equals(t + ln.tab[0] + 1, ln.tab[1] - ln.tab[0] - 1, "reference genome", 16);
    if (P.reference_only && !is_ref) return 0;
    const int32_t n_ftp = ln.tab[8] - ln.tab[7] - 1;
    if (n_ftp <= 0) {  // the reference throws
        as_bad(P, (uint32_t)L);
        return 0;
    }
    *bytes = (uint32_t)((ln.tab[2] - ln.tab[1] - 1) + (ln.tab[3] - ln.tab[2] - 1) + n_ftp);
    return GS_AS_KEPT | (u64)is_ref << 40 | (u64)q << 32 | (u64)(uint32_t)lo;
}

__global__ __launch_bounds__(AS_BLOCK) void gs_as_judge_kernel(GsAsmsumParams P) {
    __shared__ u64 s_wave[AS_BLOCK / 64];
    __shared__ uint32_t s_cnt[3];  // counted, short, skipped
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t L = (int64_t)blockIdx.x * AS_BLOCK + threadIdx.x;
    u64 verdict = 0;
    uint32_t bytes = 0;
    int kind = -1;  // 0: counted, 1: short, 2: comment or empty
    AsLine ln;
    if (L < P.n_lines && as_read_slot(P, L, ln)) {
        if (ln.len == 0 || P.text[ln.ls] == '#')
            kind = 2;
        else if (ln.tabs < 19)
            kind = 1;
        else {
            kind = 0;
            if (P.high[L])
                as_bad(P, (uint32_t)L);
            else
                verdict = as_judge(P, L, ln, &bytes);
        }
    }
    if (L < P.n_lines) P.verdict[L] = verdict;
    const u64 c = __ballot(kind == 0), s = __ballot(kind == 1), k = __ballot(kind == 2);
    if ((threadIdx.x & 63) == 0) {
        if (c) atomicAdd(&s_cnt[0], (uint32_t)__popcll(c));
        if (s) atomicAdd(&s_cnt[1], (uint32_t)__popcll(s));
        if (k) atomicAdd(&s_cnt[2], (uint32_t)__popcll(k));
    }
    u64 total;
    gs_block_scan((verdict ? 1ull : 0ull) | (u64)bytes << 32, s_wave, &total);  // (its barrier covers s_cnt too)
    if (threadIdx.x == 0) {
        P.line_blk[blockIdx.x] = total;
        if (s_cnt[0]) atomicAdd(&P.chunk[GS_AS_C_COUNTED], (u64)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&P.chunk[GS_AS_C_SHORT], (u64)s_cnt[1]);
        if (s_cnt[2]) atomicAdd(&P.chunk[GS_AS_C_SKIPPED], (u64)s_cnt[2]);
        if (total) {
            atomicAdd(&P.chunk[GS_AS_C_KEPT], total & 0xffffffffull);
            atomicAdd(&P.chunk[GS_AS_C_POOL], total >> 32);
        }
    }
}

__global__ __launch_bounds__(AS_BLOCK) void gs_as_write_kernel(GsAsmsumParams P) {
    __shared__ u64 s_wave[AS_BLOCK / 64];
    const int64_t L = (int64_t)blockIdx.x * AS_BLOCK + threadIdx.x;
    const u64 verdict = L < P.n_lines ? P.verdict[L] : 0;
    AsLine ln;
    uint32_t len[3] = {0, 0, 0};
    const bool kept = verdict != 0 && as_read_slot(P, L, ln);
    if (kept) {
        len[0] = (uint32_t)(ln.tab[2] - ln.tab[1] - 1);
        len[1] = (uint32_t)(ln.tab[3] - ln.tab[2] - 1);
        len[2] = (uint32_t)(ln.tab[8] - ln.tab[7] - 1);
    }
    const uint32_t bytes = len[0] + len[1] + len[2];
    u64 total;
    const u64 pre = gs_block_scan((kept ? 1ull : 0ull) | (u64)bytes << 32, s_wave, &total) + P.line_blk[blockIdx.x];
    if (!kept) return;
    const int64_t idx = (int64_t)(pre & 0xffffffffull), e = P.first_entry + idx;
    const u64 at = P.pool_used + (pre >> 32);
    if (e >= P.entry_cap || at + bytes > P.pool_cap) return;  // (the caller made room: never)
    GsAsmEntry out;
    out.node = (int32_t)(uint32_t)verdict;
    out.meta = (uint32_t)(verdict >> 32 & 0xffu) | (uint32_t)(verdict >> 40 & 1u) << 8;
    out.line = P.first_line + L;
    out.pool_off = at;
    out.len[0] = len[0];
    out.len[1] = len[1];
    out.len[2] = len[2];
    out.pad = 0;
    P.entries[e] = out;
    P.put_line[idx] = (uint32_t)L;
}

// 16 lanes per entry of the chunk: its three strings, back to back
__global__ __launch_bounds__(AS_BLOCK) void gs_as_gather_kernel(GsAsmsumParams P, int64_t n_put) {
    const int64_t idx = ((int64_t)blockIdx.x * AS_BLOCK + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (idx >= n_put || P.first_entry + idx >= P.entry_cap) return;
    AsLine ln;
    if (!as_read_slot(P, (int64_t)P.put_line[idx], ln)) return;
    const GsAsmEntry &e = P.entries[P.first_entry + idx];
    const uint32_t l0 = e.len[0], l1 = e.len[1], l2 = e.len[2];
    if (e.pool_off + l0 + l1 + l2 > P.pool_cap) return;
    const uint8_t *t = P.text + ln.ls;
    const uint8_t *s0 = t + ln.tab[1] + 1, *s1 = t + ln.tab[2] + 1, *s2 = t + ln.tab[7] + 1;
    uint8_t *dst = P.pool + e.pool_off;
    for (uint32_t j = sub; j < l0 + l1 + l2; j += 16) dst[j] = j < l0 ? s0[j] : j < l0 + l1 ? s1[j - l0] : s2[j - l0 - l1];
}

extern "C" hipError_t gs_launch_asmsum_tiles(const GsAsmsumParams *P, hipStream_t stream) {
    hipLaunchKernelGGL(gs_as_tiles_kernel, dim3((unsigned)P->n_tiles), dim3(AS_BLOCK), 0, stream, *P);
    return gs_launch_scan_blocks(P->tile_lt, P->n_tiles, P->scan_tot, stream);
}

extern "C" hipError_t gs_launch_asmsum_judge(const GsAsmsumParams *P, hipStream_t stream) {
    hipLaunchKernelGGL(gs_as_slots_kernel, dim3((unsigned)P->n_tiles), dim3(AS_BLOCK), 0, stream, *P);
    const int64_t n_blocks = (P->n_lines + AS_BLOCK - 1) / AS_BLOCK;
    if (n_blocks <= 0) return hipGetLastError();
    hipLaunchKernelGGL(gs_as_judge_kernel, dim3((unsigned)n_blocks), dim3(AS_BLOCK), 0, stream, *P);
    return gs_launch_scan_blocks(P->line_blk, n_blocks, P->scan_tot + 1, stream);
}

extern "C" hipError_t gs_launch_asmsum_write(const GsAsmsumParams *P, int64_t n_put, hipStream_t stream) {
    const int64_t n_blocks = (P->n_lines + AS_BLOCK - 1) / AS_BLOCK;
    if (n_blocks <= 0 || n_put <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_as_write_kernel, dim3((unsigned)n_blocks), dim3(AS_BLOCK), 0, stream, *P);
    hipLaunchKernelGGL(gs_as_gather_kernel, dim3((unsigned)((n_put * 16 + AS_BLOCK - 1) / AS_BLOCK)), dim3(AS_BLOCK), 0, stream, *P, n_put);
    return hipGetLastError();
}

// ---- the cap.  node_words: cnt | start | pick | pick_start, n_nodes + 1 words each
__global__ __launch_bounds__(256) void gs_as_node_count_kernel(const GsAsmEntry *entries, int64_t n, uint32_t *cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&cnt[entries[i].node], 1u);
}

// pick[node] = the entries of the node that survive; counts[1] += nodes with entries.  i runs to n_nodes: the word behind the last node
__global__ __launch_bounds__(256) void gs_as_pick_kernel(const uint32_t *cnt, int32_t n_nodes, int32_t max_per_node, uint32_t *pick, u64 *counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t c = 0;
    if (i < n_nodes) c = cnt[i];
    if (i <= n_nodes) pick[i] = max_per_node > 0 && c > (uint32_t)max_per_node ? (uint32_t)max_per_node : c;
    const u64 has = __ballot(c != 0);
    if ((threadIdx.x & 63) == 0 && has) atomicAdd(&counts[1], (u64)__popcll(has));
}

__global__ __launch_bounds__(256) void gs_as_key_kernel(const GsAsmEntry *entries, int64_t n, const uint32_t *cnt, int32_t max_per_node, u64 *key,
                                                        uint32_t *seq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t node = (uint32_t)entries[i].node, q = entries[i].meta & 0xffu;
    const bool cut = max_per_node > 0 && cnt[node] > (uint32_t)max_per_node;
    key[i] = (u64)node << 4 | (u64)(cut ? 10u - q : 0u);  // (a cut node: highest ordinal first)
    seq[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void gs_as_place_kernel(const u64 *key, const uint32_t *seq, int64_t n, const uint32_t *cnt, const uint32_t *start,
                                                          const uint32_t *pick, const uint32_t *pick_start, uint32_t *perm) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t node = (uint32_t)(key[p] >> 4);
    const uint32_t rank = (uint32_t)p - start[node], drop = cnt[node] - pick[node];
    if (rank >= drop) perm[pick_start[node] + rank - drop] = seq[p];
}

__global__ __launch_bounds__(64) void gs_as_total_kernel(const uint32_t *pick_start, int32_t n_nodes, u64 *counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) counts[0] = pick_start[n_nodes];
}

extern "C" hipError_t gs_asmsum_cap_bytes(int64_t n, int32_t n_nodes, size_t *tmp_bytes) {
    rocprim::double_buffer<u64> dk((u64 *)nullptr, (u64 *)nullptr);
    rocprim::double_buffer<uint32_t> dv((uint32_t *)nullptr, (uint32_t *)nullptr);
    size_t sort_bytes = 0, scan32 = 0, scan64 = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, dk, dv, (size_t)(n > 0 ? n : 1), 0, 36, (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(nullptr, scan32, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n_nodes + 1, rocprim::plus<uint32_t>(),
                                (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(nullptr, scan64, (u64 *)nullptr, (u64 *)nullptr, (u64)0, (size_t)(3 * (n > 0 ? n : 1) + 1), rocprim::plus<u64>(),
                                (hipStream_t) nullptr);
    *tmp_bytes = sort_bytes > scan32 ? sort_bytes : scan32;
    if (scan64 > *tmp_bytes) *tmp_bytes = scan64;
    return e;
}

extern "C" hipError_t gs_asmsum_cap(const GsAsmEntry *entries, int64_t n, int32_t n_nodes, int32_t max_per_node, uint32_t *node_words, u64 *key, u64 *key_alt,
                                    uint32_t *seq, uint32_t *seq_alt, void *tmp, size_t tmp_bytes, uint32_t *perm, u64 *counts, hipStream_t stream) {
    const size_t words = (size_t)n_nodes + 1;
    uint32_t *cnt = node_words, *start = cnt + words, *pick = start + words, *pick_start = pick + words;
    hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(u64), stream);
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, words * sizeof(uint32_t), stream);
    if (e != hipSuccess || n <= 0) return e;
    const unsigned grid = (unsigned)((n + 255) / 256), node_grid = (unsigned)((words + 255) / 256);
    hipLaunchKernelGGL(gs_as_node_count_kernel, dim3(grid), dim3(256), 0, stream, entries, n, cnt);
    hipLaunchKernelGGL(gs_as_pick_kernel, dim3(node_grid), dim3(256), 0, stream, cnt, n_nodes, max_per_node, pick, counts);
    size_t bytes = tmp_bytes;
    if ((e = rocprim::exclusive_scan(tmp, bytes, cnt, start, 0u, words, rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
    bytes = tmp_bytes;
    if ((e = rocprim::exclusive_scan(tmp, bytes, pick, pick_start, 0u, words, rocprim::plus<uint32_t>(), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(gs_as_key_kernel, dim3(grid), dim3(256), 0, stream, entries, n, cnt, max_per_node, key, seq);
    rocprim::double_buffer<u64> dk(key, key_alt);
    rocprim::double_buffer<uint32_t> dv(seq, seq_alt);
    bytes = tmp_bytes;
    if ((e = rocprim::radix_sort_pairs(tmp, bytes, dk, dv, (size_t)n, 0, 36, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(gs_as_place_kernel, dim3(grid), dim3(256), 0, stream, dk.current(), dv.current(), n, cnt, start, pick, pick_start, perm);
    hipLaunchKernelGGL(gs_as_total_kernel, dim3(1), dim3(64), 0, stream, pick_start, n_nodes, counts);
    return hipGetLastError();
}

// lens[3 j + k] = the bytes of string k of picked entry j; lens[3 m] = 0
__global__ __launch_bounds__(256) void gs_as_pick_len_kernel(const GsAsmEntry *entries, const uint32_t *perm, int64_t m, u64 *lens) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > 3 * m) return;
    lens[i] = i < 3 * m ? (u64)entries[perm[i / 3]].len[i % 3] : 0;
}

// 16 lanes per picked entry: the entry, and its strings to str_off[3 j]
__global__ __launch_bounds__(256) void gs_as_pick_gather_kernel(const GsAsmEntry *entries, const uint32_t *perm, int64_t m, const u64 *str_off,
                                                                const uint8_t *pool, GsAsmEntry *out, uint8_t *pool_out) {
    const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (j >= m) return;
    const GsAsmEntry &e = entries[perm[j]];
    const uint8_t *src = pool + e.pool_off;
    const u64 to = str_off[3 * j], n = str_off[3 * j + 3] - to;
    for (u64 i = sub; i < n; i += 16) pool_out[to + i] = src[i];
    if (sub == 0) {
        GsAsmEntry &o = out[j];
        o.node = e.node;
        o.meta = e.meta;
        o.line = e.line;
        o.pool_off = to;
        o.len[0] = e.len[0];
        o.len[1] = e.len[1];
        o.len[2] = e.len[2];
        o.pad = 0;
    }
}

extern "C" hipError_t gs_asmsum_pick_sizes(const GsAsmEntry *entries, const uint32_t *perm, int64_t m, u64 *lens, u64 *str_off, void *tmp, size_t tmp_bytes,
                                           hipStream_t stream) {
    const int64_t words = 3 * m + 1;
    hipLaunchKernelGGL(gs_as_pick_len_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, entries, perm, m, lens);
    size_t bytes = tmp_bytes;
    return rocprim::exclusive_scan(tmp, bytes, lens, str_off, (u64)0, (size_t)words, rocprim::plus<u64>(), stream);
}

extern "C" hipError_t gs_asmsum_pick_gather(const GsAsmEntry *entries, const uint32_t *perm, int64_t m, const u64 *str_off, const uint8_t *pool,
                                            GsAsmEntry *out, uint8_t *pool_out, hipStream_t stream) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_as_pick_gather_kernel, dim3((unsigned)((m * 16 + 255) / 256)), dim3(256), 0, stream, entries, perm, m, str_off, pool, out, pool_out);
    return hipGetLastError();
}
