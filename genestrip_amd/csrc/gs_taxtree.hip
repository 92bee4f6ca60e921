// gs_taxtree.hip -- lines of an NCBI nodes.dmp to the arrays of the tree on the device (the taxtree and taxnodes goals).
//
// The reference reads the dump on one thread: TaxTree.readNodesFromStream (C/tax/TaxTree.java:226-254) finds the first three '|'
// of every line `id \t|\t parent \t|\t rank \t|\t ...`, takes id = [0, a-1), parent = [a+2, b-1), rank = [b+2, c-1), hangs the
// node into its parent's child list in line order and TaxIdNode.initPositions (:491-502) walks the lists from the node "1".
// gs_taxparse.h restates all of it line by line, with everything it does on lines that NCBI never writes.
//
// The grammar.  A chunk is taken here only if every line of it is one of
//     "\n" alone                                                       -> an empty slot
//     at least three '|', no NUL byte, at most GS_TT_MAX_LINE bytes with its newline, [0, a-1) and [a+2, b-1) 1-9 digits
//     without a leading zero                                           -> the slot (id, parent, ordinal of the rank or -1)
// and only its last line, and only if the stream ends with it, may lack its newline.  On such lines the reference does the plain
// thing.  Anything else refuses the chunk: the handle stays as it was and the first bad line is reported.  Every line has one slot,
// at its line number, so slots are in input order without a second pass.
// Two lines with one id are inside this grammar but outside what the finish can do: gs_tt_resolve_kernel counts them and the
// handle goes through the host's child lists instead (gs_api.cpp).
//
// The scan: a thread owns 16 bytes, a block GS_TT_TILE; newlines and bars in front of every byte come from the block scan of
// gs_scan.h and gs_launch_scan_blocks over the per-tile sums; the start of a byte's line and the bars in front of that start from
// one max-scan of (line start << 32 | bars) in the block, and from the tile in front across tiles, as in gs_accmap.hip.
//   gs_tt_tiles_kernel     per tile: newlines, bars; its last newline and the bars behind it                    1 read of the text
//   gs_tt_scan_kernel      the grammar; the lane that owns a line's SECOND bar reads id and parent backwards and the rank
//                          forwards out of the LDS copy of the tile (16 bytes in front, 32 behind, global memory beyond) and
//                          writes the slot with one 16-byte store                                                1 read
//
// The finish: tree algorithms whose launch count grows with log n and not with the depth of the tree.
//   gs_tt_keys_kernel      ids and parents of the slots as one key array; rocPRIM sorts it, gs_tt_heads_kernel + a rocPRIM scan
//                          make it distinct: taxids, ascending.  A node is its index there
//   gs_tt_resolve_kernel   per line: node and parent node by search; parent, rank, line_of; a second line for a node is counted
//   gs_tt_childkey_kernel  (parent + 1) << 32 | line per node; one stable rocPRIM sort puts siblings side by side in line order
//   gs_tt_links_kernel     first child and next sibling out of the sorted order
//   gs_tt_tour_kernel      the Euler tour as a linked list: per node with a parent an edge down (2v) and an edge up (2v+1);
//                          behind down(v) comes down(first child) or up(v), behind up(v) down(next sibling) or up(parent).  The
//                          tour of the root's tree ends in END_ROOT, that of any other root in END_OTHER; the edges of a
//                          component with a cycle never end
//   gs_tt_jump_kernel      pointer jumping (Wyllie), ceil(log2(2n + 2)) rounds between two buffers: per edge the (down edges,
//                          edges) from it to the end of its list
//   gs_tt_place_kernel     an edge that ends in END_ROOT belongs to a node the root reaches: with Sd, Sa the sums at down(v), Ud
//                          the down edges at up(v) and D the down edges of the whole tour: position = D - Sd + 1,
//                          subtree = Sd - Ud, depth = 1 + Sa - 2 Sd.  Everything else: -1, -1, 0
//   gs_tt_up_kernel        ceil(log2(n + 1)) rounds of up[v] = up[up[v]]: whoever still has an ancestor after 2^rounds >= n steps
//                          stands on a cycle then, and a step of 2^rounds permutes a cycle, so gs_tt_cyc_kernel marks every
//                          node of every cycle
// select (TaxIdCollector.withDescendants twice, C/tax/TaxIdCollector.java:119-126,172-185): a node is in if its nearest requested
// ancestor-or-self r exists and no node of the path (r, node] is blocked -- without a rank, or with one below the cut -- and it has
// no excluded ancestor-or-self.  With b(x) the nearest blocked ancestor-or-self, that is b(node) == b(r).
//   gs_tt_mark_kernel, gs_tt_anc_init_kernel, gs_tt_anc_jump_kernel (ceil(log2(n + 1)) + 1 rounds, in place: a link only ever
//   moves up to the nearest marked node), gs_tt_select_kernel
// small tree (markRequired, SmallTaxTree(TaxTree), initStoreIndices): a node the root reaches is required if a flag lies in
// [position, position + subtree) of the flags in pre-order; the value index is the rank among the required nodes in pre-order.
//   gs_tt_preflag_kernel, rocPRIM scan, gs_tt_required_kernel, rocPRIM scan, gs_tt_small_kernel
// regions below (TaxIdNode.incRefSeqRegions, C/tax/TaxTree.java:517-521, counts an entry of the accession map for its node and for
// every node of the parent chain; TaxNodesFromGenbankGoal, C/goals/genbank/TaxNodesFromGenbankGoal.java:86-92, keeps the selected
// nodes whose count is below a limit): for a node the root reaches that count is the sum of the per-node counts over
// [position, position + subtree) in pre-order -- one scatter, one scan, one difference.  Sums are kept mod 2^32: a count below 2^31
// comes out exactly.  The selection is marked per node, so the nodes come out once each and in ascending index.
//   gs_tt_regions_pre_kernel, rocPRIM scan, gs_tt_regions_incl_kernel; gs_tt_mark_kernel, gs_tt_below_flag_kernel, rocPRIM scan,
//   gs_tt_below_out_kernel
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gs_launch.h"
#include "gs_params.h"
#include "gs_scan.h"

#define TT_BLOCK GS_SCAN_BLOCK
static_assert(TT_BLOCK * 16 == GS_TT_TILE, "a thread owns 16 bytes of its tile");
#define TT_TEXT0 16
#define TT_TEXT_LDS (TT_TEXT0 + GS_TT_TILE + 32)

__device__ __forceinline__ void tt_masks(const uint4 &v, uint32_t &nlm, uint32_t &barm, uint32_t &nulm) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    nlm = barm = nulm = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        nlm |= (uint32_t)(b == '\n') << i;
        barm |= (uint32_t)(b == '|') << i;
        nulm |= (uint32_t)(b == 0) << i;
    }
}

__global__ __launch_bounds__(TT_BLOCK) void gs_tt_tiles_kernel(GsTaxScanParams P) {
    __shared__ uint32_t s_cnt[4];  // newlines, bars, last newline + 1, bars behind it
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = ((size_t)blockIdx.x * TT_BLOCK + threadIdx.x) * 16;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + base);
    uint32_t nlm, barm, nulm;
    tt_masks(v, nlm, barm, nulm);
    if (nlm) {
        atomicAdd(&s_cnt[0], (uint32_t)__popc(nlm));
        atomicMax(&s_cnt[2], threadIdx.x * 16u + (32u - (uint32_t)__clz(nlm)));
    }
    if (barm) atomicAdd(&s_cnt[1], (uint32_t)__popc(barm));
    __syncthreads();
    const uint32_t last = s_cnt[2];
    uint32_t behind = 0;
    if (threadIdx.x * 16u + 16u > last) {
        const uint32_t from = last > threadIdx.x * 16u ? last - threadIdx.x * 16u : 0u;
        behind = (uint32_t)__popc(barm >> from);
    }
    if (behind) atomicAdd(&s_cnt[3], behind);
    __syncthreads();
    if (threadIdx.x == 0) {
        P.tile_lb[blockIdx.x] = (u64)s_cnt[0] | (u64)s_cnt[1] << 32;
        P.tile_tail[blockIdx.x] = last | s_cnt[3] << 16;  // (both at most GS_TT_TILE)
    }
}

// exclusive prefix maximum of v over the block (every thread arrives); s_wave: TT_BLOCK / 64 words
__device__ __forceinline__ u64 tt_block_max_scan(u64 v, u64 *s_wave) {
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

struct TtText {
    const uint8_t *lds;  // lds[off - lo] for lo <= off < hi
    const uint8_t *glob;
    int64_t lo, hi, n_bytes;
    __device__ __forceinline__ uint32_t at(int64_t off) const {  // 0 <= off; behind the chunk: a newline
        if (off >= n_bytes) return '\n';
        return off >= lo && off < hi ? lds[off - lo] : glob[off];
    }
};

__device__ __forceinline__ void tt_bad(const GsTaxScanParams &P, uint32_t line) { atomicMin(&P.status[GS_TT_BAD_LINE], line); }

// 1-9 digits without a leading zero in [a, b): the number; 0: outside the grammar
__device__ __forceinline__ int32_t tt_number(const TtText &T, int64_t a, int64_t b) {
    if (b - a < 1 || b - a > 9 || T.at(a) == '0') return 0;
    int32_t v = 0;
    for (int64_t i = a; i < b; i++) {
        const uint32_t d = T.at(i) - '0';
        if (d > 9u) return 0;
        v = v * 10 + (int32_t)d;
    }
    return v;
}

// the slot of the line that starts at ls and has its second bar at pos_b; false: outside the grammar
__device__ bool tt_judge(const GsTaxScanParams &P, const TtText &T, int64_t ls, int64_t pos_b, uint4 &slot) {
    // the first bar: id has at most nine digits and one dropped byte in front of the bar
    int64_t pos_a = ls;
    while (pos_a < pos_b && pos_a <= ls + 10 && T.at(pos_a) != '|') pos_a++;
    if (pos_a >= pos_b || T.at(pos_a) != '|') return false;
    const int32_t id = tt_number(T, ls, pos_a - 1);
    const int32_t parent = tt_number(T, pos_a + 2, pos_b - 1);
    if (id == 0 || parent == 0) return false;
    // the rank: [pos_b + 2, c - 1) where c is the third bar; a field beyond the longest name is no rank (whether the line has a
    // third bar at all is the business of the lane at its end)
    int64_t c = pos_b + 1;
    const int64_t limit = pos_b + 4 + GS_TT_RANK_BYTES;
    while (c < limit) {
        const uint32_t x = T.at(c);
        if (x == '|' || x == '\n') break;
        c++;
    }
    int32_t rank = -1;
    const int64_t len = c - 1 - (pos_b + 2);
    if (c < limit && T.at(c) == '|' && len >= 1 && len < GS_TT_RANK_BYTES) {
        uint8_t f[GS_TT_RANK_BYTES];
#pragma unroll
        for (int j = 0; j < GS_TT_RANK_BYTES; j++) f[j] = j < len ? (uint8_t)T.at(pos_b + 2 + j) : 0;
        for (int r = 0; r < GS_TT_N_RANKS && rank < 0; r++) {
            if (P.ranks->len[r] != len) continue;
            bool same = true;
#pragma unroll
            for (int j = 0; j < GS_TT_RANK_BYTES; j++) same = same && (j >= len || f[j] == P.ranks->text[r][j]);
            if (same) rank = r;
        }
    }
    slot = make_uint4((uint32_t)id, (uint32_t)parent, (uint32_t)rank, 0u);
    return true;
}

__global__ __launch_bounds__(TT_BLOCK) void gs_tt_scan_kernel(GsTaxScanParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[TT_TEXT_LDS];
    __shared__ u64 s_wave[2 * TT_BLOCK / 64];
    __shared__ uint32_t s_longest;
    const int64_t tile = blockIdx.x;
    const int64_t tile0 = tile * GS_TT_TILE;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + tile0 + threadIdx.x * 16);
    *reinterpret_cast<uint4 *>(s_text + TT_TEXT0 + threadIdx.x * 16) = v;
    if (threadIdx.x < 2)  // (the text's buffer ends 64 zero bytes behind its last tile)
        *reinterpret_cast<uint4 *>(s_text + TT_TEXT0 + GS_TT_TILE + threadIdx.x * 16) =
            *reinterpret_cast<const uint4 *>(P.text + tile0 + GS_TT_TILE + threadIdx.x * 16);
    if (threadIdx.x == 2)
        *reinterpret_cast<uint4 *>(s_text) = tile ? *reinterpret_cast<const uint4 *>(P.text + tile0 - 16) : make_uint4(0, 0, 0, 0);
    if (threadIdx.x == 3) s_longest = 0;
    __syncthreads();
    TtText T;
    T.glob = P.text;
    T.lo = tile ? tile0 - TT_TEXT0 : 0;
    T.lds = s_text + TT_TEXT0 - (tile0 - T.lo);
    T.hi = tile0 + GS_TT_TILE + 32;
    T.n_bytes = P.n_bytes;

    uint32_t nlm, barm, nulm;
    tt_masks(v, nlm, barm, nulm);
    const int64_t base = tile0 + threadIdx.x * 16;
    u64 total;
    const u64 tile_lb = P.tile_lb[tile];
    const u64 lb = gs_block_scan((u64)__popc(nlm) | (u64)__popc(barm) << 32, s_wave, &total) + tile_lb;
    uint32_t L = (uint32_t)lb, g = (uint32_t)(lb >> 32);
    u64 mine = 0;
    if (nlm) {
        const int i = 31 - __clz(nlm);
        mine = (u64)(base + i + 1) << 32 | (u64)(g + (uint32_t)__popc(barm & ((1u << i) - 1u)));
    }
    const u64 start = tt_block_max_scan(mine, s_wave + TT_BLOCK / 64);
    int64_t ls = 0;
    uint32_t g0 = 0;
    if (start) {
        ls = (int64_t)(start >> 32);
        g0 = (uint32_t)start;
    } else if (tile) {  // (without a newline in the tile in front, the line is above GS_TT_MAX_LINE whatever ls says)
        const uint32_t tt = P.tile_tail[tile - 1];
        ls = tile0 - GS_TT_TILE + (tt & 0xffffu);
        g0 = (uint32_t)(tile_lb >> 32) - (tt >> 16);
    }

    uint32_t longest = 0;
    for (int i = 0; i < 16 && base + i < P.n_bytes; i++) {
        const int64_t off = base + i;
        bool line_ends = false;
        if (nlm >> i & 1) {
            line_ends = true;
        } else {
            if (barm >> i & 1) {
                if (g - g0 == 1) {
                    uint4 slot;
                    const int64_t at = P.first_line + (int64_t)L;
                    if (!tt_judge(P, T, ls, off, slot))
                        tt_bad(P, L);
                    else if (at < P.slot_cap)
                        P.slots[at] = slot;
                }
                g++;
            } else if (nulm >> i & 1) {
                tt_bad(P, L);
            }
            if (off == P.n_bytes - 1) {  // the unterminated tail: a line if the stream ends here
                if (!P.last) tt_bad(P, L);
                line_ends = true;
            }
        }
        if (line_ends) {
            const uint32_t len = (uint32_t)(off - ls + 1);
            longest = len > longest ? len : longest;
            if (len > GS_TT_MAX_LINE)
                tt_bad(P, L);
            else if (!(len == 1 && (nlm >> i & 1)) && g - g0 < 3)
                tt_bad(P, L);
            L++;
            ls = off + 1;
            g0 = g;
        }
    }
    if (longest) atomicMax(&s_longest, longest);
    __syncthreads();
    if (threadIdx.x == 0 && s_longest) atomicMax(&P.status[GS_TT_LONGEST], s_longest);
}

__device__ __forceinline__ int32_t tt_find(const int32_t *taxids, int32_t n, int32_t id);

// ---- names.dmp: TaxTree.readNamesFromStream (C/tax/TaxTree.java:196-216).  The grammar: every line is "\n" alone or has two
// bars and more, no NUL byte and at most GS_TT_MAX_LINE bytes; an id [0, a-1) that is no 1-9 digits without a leading zero, or that
// names no node, makes a line the rules skip (the lookup does not create); a line of a known node has a name [a+2, b-1) of zero
// bytes or more.  MODE 0 judges the chunk and writes nothing.  MODE 1 (only behind a MODE 0 that refused nothing): one 64-bit
// atomicMax per line on its node's key decides among the lines of the whole stream.  MODE 2: a line whose key stands in its node
// takes room in the pool with one atomicAdd and copies its name there; an earlier winner's bytes stay behind as dead bytes.
__constant__ uint8_t tt_scientific[16] = {'s', 'c', 'i', 'e', 'n', 't', 'i', 'f', 'i', 'c', ' ', 'n', 'a', 'm', 'e', 0};

template <int MODE>
__device__ void tt_names_judge(const GsTaxScanParams &P, const TtText &T, int64_t ls, int64_t pos_b, uint32_t L) {
    int64_t pos_a = ls;
    while (pos_a < pos_b && T.at(pos_a) != '|') pos_a++;
    const int32_t id = tt_number(T, ls, pos_a - 1);  // (0 also for a bar in column 0 or 1)
    if (id == 0) return;
    const int32_t node = tt_find(P.taxids, P.n_nodes, id);
    if (node >= P.n_nodes || P.taxids[node] != id) return;
    const int64_t len = pos_b - 1 - (pos_a + 2);
    if (len < 0) {
        if (MODE == 0) tt_bad(P, L);
        return;
    }
    if (MODE == 0) return;
    // "scientific name" anywhere in the line
    bool sci = false;
    const int64_t limit = ls + GS_TT_MAX_LINE;
    for (int64_t i = ls; i < limit && !sci; i++) {
        const uint32_t c = T.at(i);
        if (c == '\n') break;
        if (c != 's') continue;
        int j = 1;
        while (j < 15 && T.at(i + j) == (uint32_t)tt_scientific[j]) j++;
        sci = j == 15;
    }
    const u64 key = GS_TT_NAME_KEY(sci, P.first_line + (int64_t)L + 1);
    if (MODE == 1) {
        atomicMax(&P.win[node], key);
    } else if (P.win[node] == key) {
        const u64 off = atomicAdd(P.pool_used, (u64)len);
        P.name_off[node] = off;
        P.name_len[node] = (uint32_t)len;
        for (int64_t j = 0; j < len; j++) P.pool[off + j] = (uint8_t)T.at(pos_a + 2 + j);
    }
}

template <int MODE>
__global__ __launch_bounds__(TT_BLOCK) void gs_tt_names_kernel(GsTaxScanParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[TT_TEXT_LDS];
    __shared__ u64 s_wave[2 * TT_BLOCK / 64];
    __shared__ uint32_t s_longest;
    const int64_t tile = blockIdx.x;
    const int64_t tile0 = tile * GS_TT_TILE;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + tile0 + threadIdx.x * 16);
    *reinterpret_cast<uint4 *>(s_text + TT_TEXT0 + threadIdx.x * 16) = v;
    if (threadIdx.x < 2)
        *reinterpret_cast<uint4 *>(s_text + TT_TEXT0 + GS_TT_TILE + threadIdx.x * 16) =
            *reinterpret_cast<const uint4 *>(P.text + tile0 + GS_TT_TILE + threadIdx.x * 16);
    if (threadIdx.x == 2)
        *reinterpret_cast<uint4 *>(s_text) = tile ? *reinterpret_cast<const uint4 *>(P.text + tile0 - 16) : make_uint4(0, 0, 0, 0);
    if (threadIdx.x == 3) s_longest = 0;
    __syncthreads();
    TtText T;
    T.glob = P.text;
    T.lo = tile ? tile0 - TT_TEXT0 : 0;
    T.lds = s_text + TT_TEXT0 - (tile0 - T.lo);
    T.hi = tile0 + GS_TT_TILE + 32;
    T.n_bytes = P.n_bytes;

    uint32_t nlm, barm, nulm;
    tt_masks(v, nlm, barm, nulm);
    const int64_t base = tile0 + threadIdx.x * 16;
    u64 total;
    const u64 tile_lb = P.tile_lb[tile];
    const u64 lb = gs_block_scan((u64)__popc(nlm) | (u64)__popc(barm) << 32, s_wave, &total) + tile_lb;
    uint32_t L = (uint32_t)lb, g = (uint32_t)(lb >> 32);
    u64 mine = 0;
    if (nlm) {
        const int i = 31 - __clz(nlm);
        mine = (u64)(base + i + 1) << 32 | (u64)(g + (uint32_t)__popc(barm & ((1u << i) - 1u)));
    }
    const u64 start = tt_block_max_scan(mine, s_wave + TT_BLOCK / 64);
    int64_t ls = 0;
    uint32_t g0 = 0;
    if (start) {
        ls = (int64_t)(start >> 32);
        g0 = (uint32_t)start;
    } else if (tile) {
        const uint32_t tt = P.tile_tail[tile - 1];
        ls = tile0 - GS_TT_TILE + (tt & 0xffffu);
        g0 = (uint32_t)(tile_lb >> 32) - (tt >> 16);
    }

    uint32_t longest = 0;
    for (int i = 0; i < 16 && base + i < P.n_bytes; i++) {
        const int64_t off = base + i;
        bool line_ends = false;
        if (nlm >> i & 1) {
            line_ends = true;
        } else {
            if (barm >> i & 1) {
                if (g - g0 == 1) tt_names_judge<MODE>(P, T, ls, off, L);
                g++;
            } else if (MODE == 0 && (nulm >> i & 1)) {
                tt_bad(P, L);
            }
            if (off == P.n_bytes - 1) {
                if (MODE == 0 && !P.last) tt_bad(P, L);
                line_ends = true;
            }
        }
        if (line_ends) {
            const uint32_t len = (uint32_t)(off - ls + 1);
            longest = len > longest ? len : longest;
            if (MODE == 0 && (len > GS_TT_MAX_LINE || (!(len == 1 && (nlm >> i & 1)) && g - g0 < 2))) tt_bad(P, L);
            L++;
            ls = off + 1;
            g0 = g;
        }
    }
    if (MODE == 0) {
        if (longest) atomicMax(&s_longest, longest);
        __syncthreads();
        if (threadIdx.x == 0 && s_longest) atomicMax(&P.status[GS_TT_LONGEST], s_longest);
    }
}

// mode 0: the grammar; 1: the votes; 2: the names of the winners into the pool
extern "C" hipError_t gs_launch_taxtree_names(const GsTaxScanParams *P, int mode, hipStream_t stream) {
    const dim3 grid((unsigned)P->n_tiles), block(TT_BLOCK);
    if (mode == 0) hipLaunchKernelGGL(gs_tt_names_kernel<0>, grid, block, 0, stream, *P);
    if (mode == 1) hipLaunchKernelGGL(gs_tt_names_kernel<1>, grid, block, 0, stream, *P);
    if (mode == 2) hipLaunchKernelGGL(gs_tt_names_kernel<2>, grid, block, 0, stream, *P);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_taxtree_tiles(const GsTaxScanParams *P, hipStream_t stream) {
    hipLaunchKernelGGL(gs_tt_tiles_kernel, dim3((unsigned)P->n_tiles), dim3(TT_BLOCK), 0, stream, *P);
    return gs_launch_scan_blocks(P->tile_lb, P->n_tiles, P->scan_tot, stream);
}

extern "C" hipError_t gs_launch_taxtree_scan(const GsTaxScanParams *P, hipStream_t stream) {
    hipLaunchKernelGGL(gs_tt_scan_kernel, dim3((unsigned)P->n_tiles), dim3(TT_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

// ---- the finish
#define TT_LAUNCH(kernel, n, stream, ...) hipLaunchKernelGGL(kernel, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, stream, __VA_ARGS__)

__global__ __launch_bounds__(256) void gs_tt_keys_kernel(const uint4 *slots, int64_t m, uint32_t *keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const uint4 s = slots[i];
    keys[i] = s.x;
    keys[m + i] = s.x ? s.y : 0u;
}

// head[i] = 1 if sorted key i is not 0 and differs from the one in front of it
__global__ __launch_bounds__(256) void gs_tt_heads_kernel(const uint32_t *keys, int64_t n, uint32_t *head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    head[i] = k != 0 && (i == 0 || keys[i - 1] != k);
}

// taxids[rank of head i] = keys[i]; idx: the exclusive scan of head
__global__ __launch_bounds__(256) void gs_tt_distinct_kernel(const uint32_t *keys, const uint32_t *idx, int64_t n, int32_t *taxids) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (k != 0 && (i == 0 || keys[i - 1] != k)) taxids[idx[i]] = (int32_t)k;
}

__device__ __forceinline__ int32_t tt_find(const int32_t *taxids, int32_t n, int32_t id) {  // (id is among them)
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (taxids[mid] < id)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// parent, rank, line_of arrive as -1.  counts[0]: lines whose node had a line before
__global__ __launch_bounds__(256) void gs_tt_resolve_kernel(const uint4 *slots, int64_t m, GsTaxTreeArrays A, u64 *counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool dup = false;
    if (i < m) {
        const uint4 s = slots[i];
        if (s.x) {
            const int32_t a = tt_find(A.taxids, A.n, (int32_t)s.x), b = tt_find(A.taxids, A.n, (int32_t)s.y);
            dup = atomicCAS(&A.line_of[a], -1, (int32_t)i) != -1;
            if (!dup) {
                A.parent[a] = a == b ? -1 : b;
                A.rank[a] = (int32_t)s.z;
            }
        }
    }
    const u64 d = __ballot(dup);
    if ((threadIdx.x & 63) == 0 && d) atomicAdd(&counts[0], (u64)__popcll(d));
}

__global__ __launch_bounds__(256) void gs_tt_childkey_kernel(GsTaxTreeArrays A, u64 *key, uint32_t *val) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (v >= A.n) return;
    key[v] = (u64)(uint32_t)(A.parent[v] + 1) << 32 | (u64)(uint32_t)A.line_of[v];
    val[v] = (uint32_t)v;
}

// first_child and next_sib arrive as -1
__global__ __launch_bounds__(256) void gs_tt_links_kernel(const u64 *key, const uint32_t *ord, int32_t n, int32_t *first_child, int32_t *next_sib) {
    const int32_t r = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (r >= n) return;
    const uint32_t p1 = (uint32_t)(key[r] >> 32);
    if (p1 == 0) return;
    const int32_t v = (int32_t)ord[r];
    if (r + 1 < n && (uint32_t)(key[r + 1] >> 32) == p1) next_sib[v] = (int32_t)ord[r + 1];
    if (r == 0 || (uint32_t)(key[r - 1] >> 32) != p1) first_child[p1 - 1] = v;
}

// 2n + 2 edges: succ, val = down edges << 32 | edges
__global__ __launch_bounds__(256) void gs_tt_tour_kernel(GsTaxTreeArrays A, const int32_t *first_child, const int32_t *next_sib, uint32_t *succ, u64 *val) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    const uint32_t end_root = 2u * (uint32_t)A.n, end_other = end_root + 1;
    if (v == A.n) {
        succ[end_root] = end_root;
        succ[end_other] = end_other;
        val[end_root] = val[end_other] = 0;
    }
    if (v >= A.n) return;
    const int32_t p = A.parent[v];
    if (p < 0) {
        succ[2 * v] = succ[2 * v + 1] = end_other;
        val[2 * v] = val[2 * v + 1] = 0;
        return;
    }
    const int32_t fc = first_child[v], ns = next_sib[v];
    succ[2 * v] = fc >= 0 ? 2u * (uint32_t)fc : 2u * (uint32_t)v + 1;
    val[2 * v] = (u64)1 << 32 | 1u;
    uint32_t s;
    if (ns >= 0)
        s = 2u * (uint32_t)ns;
    else if (A.parent[p] < 0)
        s = p == A.root ? end_root : end_other;
    else
        s = 2u * (uint32_t)p + 1;
    succ[2 * v + 1] = s;
    val[2 * v + 1] = 1u;
}

__global__ __launch_bounds__(256) void gs_tt_jump_kernel(const uint32_t *succ, const u64 *val, int64_t n_edges, uint32_t *succ_out, u64 *val_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const uint32_t s = succ[e];
    val_out[e] = val[e] + val[s];
    succ_out[e] = succ[s];
}

// counts[1]: nodes the root reaches; counts[2]: the deepest of them
__global__ __launch_bounds__(256) void gs_tt_place_kernel(GsTaxTreeArrays A, const int32_t *first_child, const uint32_t *succ, const u64 *val, u64 *counts) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    const uint32_t end_root = 2u * (uint32_t)A.n;
    int32_t depth = -1, pos = -1, sub = 0;
    if (v < A.n) {
        const int32_t rfc = first_child[A.root];
        const int32_t D = rfc >= 0 ? (int32_t)(val[2 * rfc] >> 32) : 0;
        if (v == A.root) {
            depth = 0;
            pos = 0;
            sub = D + 1;
        } else if (A.parent[v] >= 0 && succ[2 * v] == end_root) {
            const u64 dn = val[2 * v];
            const int32_t sd = (int32_t)(dn >> 32), sa = (int32_t)(uint32_t)dn, ud = (int32_t)(val[2 * v + 1] >> 32);
            pos = D - sd + 1;
            sub = sd - ud;
            depth = 1 + sa - 2 * sd;
        }
        A.depth[v] = depth;
        A.position[v] = pos;
        A.subtree[v] = sub;
        if (pos >= 0) A.node_at[pos] = v;
    }
    const u64 reach = __ballot(pos >= 0);
    int32_t deepest = depth;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int32_t x = __shfl_xor(deepest, d);
        deepest = x > deepest ? x : deepest;
    }
    if ((threadIdx.x & 63) == 0 && reach) {
        atomicAdd(&counts[1], (u64)__popcll(reach));
        atomicMax(&counts[2], (u64)deepest);
    }
}

__global__ __launch_bounds__(256) void gs_tt_up_kernel(const int32_t *up, int32_t n, int32_t *up_out) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (v >= n) return;
    const int32_t u = up[v];
    up_out[v] = u < 0 ? -1 : up[u];
}

// cyc arrives as 0.  counts[3]: nodes that stand below or on a cycle
__global__ __launch_bounds__(256) void gs_tt_cyc_kernel(const int32_t *up, int32_t n, uint8_t *cyc, u64 *counts) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    const bool on = v < n && up[v] >= 0;
    if (on) cyc[up[v]] = 1;
    const u64 c = __ballot(on);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&counts[3], (u64)__popcll(c));
}

static inline int tt_log2_ceil(u64 x) {
    int k = 0;
    while (((u64)1 << k) < x) k++;
    return k;
}

extern "C" hipError_t gs_taxtree_sort_bytes(int64_t n_keys, size_t *tmp_bytes) {
    const size_t n = (size_t)(n_keys > 0 ? n_keys : 1);
    size_t a = 0, b = 0, c = 0;
    rocprim::double_buffer<uint32_t> dk((uint32_t *)nullptr, (uint32_t *)nullptr);
    hipError_t e = rocprim::radix_sort_keys(nullptr, a, dk, n, 0, 32, (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    rocprim::double_buffer<u64> dk2((u64 *)nullptr, (u64 *)nullptr);
    rocprim::double_buffer<uint32_t> dv((uint32_t *)nullptr, (uint32_t *)nullptr);
    e = rocprim::radix_sort_pairs(nullptr, b, dk2, dv, n, 0, 64, (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(nullptr, c, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, n, rocprim::plus<uint32_t>(), (hipStream_t) nullptr);
    *tmp_bytes = a > b ? (a > c ? a : c) : (b > c ? b : c);
    return e;
}

// slots[m] -> keys sorted and made distinct: taxids[<= 2m] and *n_out on the device (counts[4]).  keys, keys_alt, head, idx: 2m words each
extern "C" hipError_t gs_taxtree_distinct(const uint4 *slots, int64_t m, uint32_t *keys, uint32_t *keys_alt, uint32_t *head, uint32_t *idx, void *tmp,
                                          size_t tmp_bytes, int32_t *taxids, u64 *counts, hipStream_t stream) {
    if (m <= 0) return hipSuccess;
    const int64_t n2 = 2 * m;
    TT_LAUNCH(gs_tt_keys_kernel, m, stream, slots, m, keys);
    rocprim::double_buffer<uint32_t> dk(keys, keys_alt);
    hipError_t e = rocprim::radix_sort_keys(tmp, tmp_bytes, dk, (size_t)n2, 0, 32, stream);
    if (e != hipSuccess) return e;
    const uint32_t *sorted = dk.current();
    TT_LAUNCH(gs_tt_heads_kernel, n2, stream, sorted, n2, head);
    e = rocprim::exclusive_scan(tmp, tmp_bytes, head, idx, 0u, (size_t)n2, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    TT_LAUNCH(gs_tt_distinct_kernel, n2, stream, sorted, idx, n2, taxids);
    // the number of nodes: idx of the last key + its head, left where the host reads it
    e = hipMemcpyAsync((uint32_t *)&counts[4], idx + n2 - 1, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return e;
    return hipMemcpyAsync((uint32_t *)&counts[4] + 1, head + n2 - 1, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
}

// parent, rank, line_of of the n nodes; counts[0]: duplicates
extern "C" hipError_t gs_taxtree_resolve(const uint4 *slots, int64_t m, const GsTaxTreeArrays *A, u64 *counts, hipStream_t stream) {
    const size_t bytes = (size_t)A->n * sizeof(int32_t);
    hipError_t e = hipMemsetAsync(A->parent, 0xff, bytes, stream);
    if (e == hipSuccess) e = hipMemsetAsync(A->rank, 0xff, bytes, stream);
    if (e == hipSuccess) e = hipMemsetAsync(A->line_of, 0xff, bytes, stream);
    if (e != hipSuccess) return e;
    TT_LAUNCH(gs_tt_resolve_kernel, m, stream, slots, m, *A, counts);
    return hipGetLastError();
}

// child order by one stable sort; key, key_alt: n u64; ord, ord_alt, first_child, next_sib: n words.  *ord_out, *key_out: the sorted buffers
extern "C" hipError_t gs_taxtree_children(const GsTaxTreeArrays *A, u64 *key, u64 *key_alt, uint32_t *ord, uint32_t *ord_alt, void *tmp, size_t tmp_bytes,
                                          int32_t *first_child, int32_t *next_sib, hipStream_t stream) {
    const int32_t n = A->n;
    TT_LAUNCH(gs_tt_childkey_kernel, n, stream, *A, key, ord);
    rocprim::double_buffer<u64> dk(key, key_alt);
    rocprim::double_buffer<uint32_t> dv(ord, ord_alt);
    hipError_t e = rocprim::radix_sort_pairs(tmp, tmp_bytes, dk, dv, (size_t)n, 0, 64, stream);
    if (e == hipSuccess) e = hipMemsetAsync(first_child, 0xff, (size_t)n * sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(next_sib, 0xff, (size_t)n * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    TT_LAUNCH(gs_tt_links_kernel, n, stream, dk.current(), dv.current(), n, first_child, next_sib);
    return hipGetLastError();
}

// depth, position, subtree, node_at, cyc; succ, succ_alt: 2n + 2 words; val, val_alt: 2n + 2 u64; up, up_alt: n words.
// counts[1]: reached, counts[2]: deepest, counts[3]: nodes on or below a cycle
extern "C" hipError_t gs_taxtree_place(const GsTaxTreeArrays *A, const int32_t *first_child, const int32_t *next_sib, uint32_t *succ, uint32_t *succ_alt, u64 *val,
                                       u64 *val_alt, int32_t *up, int32_t *up_alt, u64 *counts, hipStream_t stream) {
    const int32_t n = A->n;
    const int64_t n_edges = 2 * (int64_t)n + 2;
    TT_LAUNCH(gs_tt_tour_kernel, n + 1, stream, *A, first_child, next_sib, succ, val);
    const int rounds = tt_log2_ceil((u64)n_edges);
    for (int r = 0; r < rounds; r++) {
        TT_LAUNCH(gs_tt_jump_kernel, n_edges, stream, succ, val, n_edges, succ_alt, val_alt);
        uint32_t *s = succ;
        succ = succ_alt;
        succ_alt = s;
        u64 *w = val;
        val = val_alt;
        val_alt = w;
    }
    TT_LAUNCH(gs_tt_place_kernel, n, stream, *A, first_child, succ, val, counts);
    hipError_t e = hipMemcpyAsync(up, A->parent, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(A->cyc, 0, (size_t)n, stream);
    if (e != hipSuccess) return e;
    const int up_rounds = tt_log2_ceil((u64)n + 1);
    for (int r = 0; r < up_rounds; r++) {
        TT_LAUNCH(gs_tt_up_kernel, n, stream, up, n, up_alt);
        int32_t *s = up;
        up = up_alt;
        up_alt = s;
    }
    TT_LAUNCH(gs_tt_cyc_kernel, n, stream, up, n, A->cyc, counts);
    return hipGetLastError();
}

// ---- select
// Rank.level over ordinals (C/tax/Rank.java:104-112,176-184)
__device__ __forceinline__ int tt_level(int ordinal) {
    if (ordinal == 32 || ordinal == 33) return -1;
    if (ordinal == 34) return 5 * 20 + 10;
    if (ordinal == 35) return 18 * 20 + 10;
    return ordinal * 20;
}

// marks arrive as 0: bit 0 requested, bit 1 excluded
__global__ __launch_bounds__(256) void gs_tt_mark_kernel(const int32_t *list, int64_t n_list, uint8_t bit, uint8_t *marks) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_list) return;
    // (a byte per node and one bit per launch: two lists never write one byte at the same time)
    marks[list[i]] |= bit;
}

// bit 2 of marks: blocked.  anc[k * n + v]: v itself if it carries mark k, else its parent
__global__ __launch_bounds__(256) void gs_tt_anc_init_kernel(GsTaxTreeArrays A, int cut, uint8_t *marks, int32_t *anc) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (v >= A.n) return;
    const int32_t rank = A.rank[v];
    bool blocked = false;
    if (cut >= 0) {
        const int a = rank < 0 ? -1 : tt_level(rank), b = tt_level(cut);
        blocked = rank < 0 || (a != -1 && b != -1 && a > b);
    }
    const uint8_t m = (uint8_t)(marks[v] | (blocked ? 4 : 0));
    marks[v] = m;
    const int32_t p = A.parent[v];
#pragma unroll
    for (int k = 0; k < 3; k++) anc[(size_t)k * A.n + v] = (m >> k & 1) ? v : p;
}

__global__ __launch_bounds__(256) void gs_tt_anc_jump_kernel(int32_t n, const uint8_t *marks, int32_t *anc) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (v >= n) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int32_t *a = anc + (size_t)k * n;
        const int32_t u = a[v];
        if (u >= 0 && !(marks[u] >> k & 1)) a[v] = a[u];
    }
}

__global__ __launch_bounds__(256) void gs_tt_select_kernel(int32_t n, const uint8_t *marks, const int32_t *anc, uint8_t *out, u64 *count) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    bool in = false;
    if (v < n) {
        auto nearest = [&](int k, int32_t x) {
            const int32_t u = anc[(size_t)k * n + x];
            return u >= 0 && (marks[u] >> k & 1) ? u : -1;
        };
        const int32_t r = nearest(0, v);
        in = r >= 0 && nearest(1, v) < 0 && nearest(2, v) == nearest(2, r);
        out[v] = in;
    }
    const u64 c = __ballot(in);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (u64)__popcll(c));
}

// requested, excluded: node indices on the device; marks: n bytes; anc: 3n words; out: n bytes; *count arrives as 0
extern "C" hipError_t gs_launch_taxtree_select(const GsTaxTreeArrays *A, const int32_t *requested, int64_t n_req, const int32_t *excluded, int64_t n_exc, int cut,
                                               uint8_t *marks, int32_t *anc, uint8_t *out, u64 *count, hipStream_t stream) {
    const int32_t n = A->n;
    hipError_t e = hipMemsetAsync(marks, 0, (size_t)n, stream);
    if (e != hipSuccess) return e;
    if (n_req > 0) TT_LAUNCH(gs_tt_mark_kernel, n_req, stream, requested, n_req, (uint8_t)1, marks);
    if (n_exc > 0) TT_LAUNCH(gs_tt_mark_kernel, n_exc, stream, excluded, n_exc, (uint8_t)2, marks);
    TT_LAUNCH(gs_tt_anc_init_kernel, n, stream, *A, cut, marks, anc);
    const int rounds = tt_log2_ceil((u64)n + 1) + 1;
    for (int r = 0; r < rounds; r++) TT_LAUNCH(gs_tt_anc_jump_kernel, n, stream, n, marks, anc);
    TT_LAUNCH(gs_tt_select_kernel, n, stream, n, marks, anc, out, count);
    return hipGetLastError();
}

// ---- small tree
// pre[p] = 1 if the node at position p is flagged (flag8 or flag32, whichever is not null; > 0 means flagged)
__global__ __launch_bounds__(256) void gs_tt_preflag_kernel(GsTaxTreeArrays A, int32_t n_reach, const uint8_t *flag8, const int32_t *flag32, uint32_t *pre) {
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_reach) return;
    const int32_t v = A.node_at[p];
    pre[p] = flag8 ? flag8[v] != 0 : flag32[v] > 0;
}

// sum: the exclusive scan of pre (n_reach entries); req[p] = 1 if a flag lies in the subtree of the node at p, or p is the root
__global__ __launch_bounds__(256) void gs_tt_required_kernel(GsTaxTreeArrays A, int32_t n_reach, const uint32_t *pre, const uint32_t *sum, uint32_t *req) {
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_reach) return;
    const int32_t last = p + A.subtree[A.node_at[p]] - 1;  // the last position of the subtree
    req[p] = p == 0 || sum[last] + pre[last] > sum[p];
}

// vi: the exclusive scan of req
__global__ __launch_bounds__(256) void gs_tt_small_kernel(GsTaxTreeArrays A, int32_t n_reach, const uint32_t *req, const uint32_t *vi, int32_t *node_of_vi,
                                                          int32_t *parent_vi, int32_t *depth, int32_t *position) {
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_reach || !req[p]) return;
    const int32_t v = A.node_at[p], i = (int32_t)vi[p];
    node_of_vi[i] = v;
    parent_vi[i] = p == 0 ? -1 : (int32_t)vi[A.position[A.parent[v]]];
    depth[i] = A.depth[v];
    position[i] = p;
}

// pre, sum, req, vi: n_reach words each; out arrays: n_reach words each; n_small = vi[n_reach - 1] + req[n_reach - 1] (the root makes it >= 1)
extern "C" hipError_t gs_launch_taxtree_small(const GsTaxTreeArrays *A, int32_t n_reach, const uint8_t *flag8, const int32_t *flag32, uint32_t *pre, uint32_t *sum,
                                              uint32_t *req, uint32_t *vi, void *tmp, size_t tmp_bytes, int32_t *node_of_vi, int32_t *parent_vi, int32_t *depth,
                                              int32_t *position, hipStream_t stream) {
    TT_LAUNCH(gs_tt_preflag_kernel, n_reach, stream, *A, n_reach, flag8, flag32, pre);
    hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, pre, sum, 0u, (size_t)n_reach, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    TT_LAUNCH(gs_tt_required_kernel, n_reach, stream, *A, n_reach, pre, sum, req);
    e = rocprim::exclusive_scan(tmp, tmp_bytes, req, vi, 0u, (size_t)n_reach, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    TT_LAUNCH(gs_tt_small_kernel, n_reach, stream, *A, n_reach, req, vi, node_of_vi, parent_vi, depth, position);
    return hipGetLastError();
}

// ---- regions with ancestors, and the selected nodes below a limit
// pre[p] = the regions of the node at position p
__global__ __launch_bounds__(256) void gs_tt_regions_pre_kernel(GsTaxTreeArrays A, int32_t n_reach, const int32_t *regions, uint32_t *pre) {
    const int32_t p = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_reach) return;
    pre[p] = (uint32_t)regions[A.node_at[p]];
}

// sum: the exclusive scan of pre.  incl[v] = the regions in [position, position + subtree) for a node the root reaches; its own
// regions else: what hangs below such a node is added on the host
__global__ __launch_bounds__(256) void gs_tt_regions_incl_kernel(GsTaxTreeArrays A, const int32_t *regions, const uint32_t *pre, const uint32_t *sum, int32_t *incl) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (v >= A.n) return;
    const int32_t p = A.position[v];
    if (p < 0) {
        incl[v] = regions[v];
        return;
    }
    const int32_t last = p + A.subtree[v] - 1;
    incl[v] = (int32_t)(sum[last] + pre[last] - sum[p]);
}

// marks[v] != 0: v is in the selection.  flag[v] = 1 if it is, has the rank asked for (check_rank < 0: any) and incl[v] < limit
__global__ __launch_bounds__(256) void gs_tt_below_flag_kernel(GsTaxTreeArrays A, const uint8_t *marks, const int32_t *incl, int32_t limit, int check_rank,
                                                               uint32_t *flag) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (v >= A.n) return;
    flag[v] = marks[v] && (check_rank < 0 || A.rank[v] == check_rank) && incl[v] < limit;
}

// idx: the exclusive scan of flag
__global__ __launch_bounds__(256) void gs_tt_below_out_kernel(int32_t n, const uint32_t *flag, const uint32_t *idx, int32_t *out) {
    const int32_t v = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (v >= n || !flag[v]) return;
    out[idx[v]] = v;
}

// incl[n] out of regions[n] (device); pre, sum: n_reach words each; tmp as gs_taxtree_sort_bytes(n) says
extern "C" hipError_t gs_launch_taxtree_regions(const GsTaxTreeArrays *A, int32_t n_reach, const int32_t *regions, uint32_t *pre, uint32_t *sum, void *tmp,
                                                size_t tmp_bytes, int32_t *incl, hipStream_t stream) {
    if (n_reach > 0) {
        TT_LAUNCH(gs_tt_regions_pre_kernel, n_reach, stream, *A, n_reach, regions, pre);
        hipError_t e = rocprim::exclusive_scan(tmp, tmp_bytes, pre, sum, 0u, (size_t)n_reach, rocprim::plus<uint32_t>(), stream);
        if (e != hipSuccess) return e;
    }
    TT_LAUNCH(gs_tt_regions_incl_kernel, A->n, stream, *A, regions, pre, sum, incl);
    return hipGetLastError();
}

// selected: n_sel node indices on the device; marks: n bytes; flag, idx: n words each; out: n words, filled in ascending node
// index; how many: idx[n - 1] + flag[n - 1]
extern "C" hipError_t gs_launch_taxtree_below(const GsTaxTreeArrays *A, const int32_t *selected, int64_t n_sel, const int32_t *incl, int32_t limit,
                                              int check_rank, uint8_t *marks, uint32_t *flag, uint32_t *idx, void *tmp, size_t tmp_bytes, int32_t *out,
                                              hipStream_t stream) {
    const int32_t n = A->n;
    hipError_t e = hipMemsetAsync(marks, 0, (size_t)n, stream);
    if (e != hipSuccess) return e;
    if (n_sel > 0) TT_LAUNCH(gs_tt_mark_kernel, n_sel, stream, selected, n_sel, (uint8_t)1, marks);
    TT_LAUNCH(gs_tt_below_flag_kernel, n, stream, *A, marks, incl, limit, check_rank, flag);
    e = rocprim::exclusive_scan(tmp, tmp_bytes, flag, idx, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    TT_LAUNCH(gs_tt_below_out_kernel, n, stream, n, flag, idx, out);
    return hipGetLastError();
}
