// gs_krakencount.hip -- Kraken-style output lines counted per tax id on the device (the krakencount goal).
//
// The reference reads such a file on one thread: KrakenResultProcessor.process (C/kraken/KrakenResultProcessor.java:74-179) splits
// every line `flag \t descriptor \t class \t size \t taxid:count taxid:count ...` and KrakenResCountGoal's listener
// (C/goals/kraken/KrakenResCountGoal.java:133-157) keeps three counters per tax id: kmers (the counts of its tokens), reads (lines
// of its class that hold at least one counted token) and kmersInMatchingReads (the count of a line's FIRST counted token where that
// token's tax id is the line's class).  Tokens whose tax id starts with 'A' are not counted.
//
// A chunk is counted here only if every line of it (up to its first empty line, where the reference stops reading) is inside a
// grammar on which the reference's state machine does exactly the above and nothing else:
//   * exactly four tabs; no blank in front of the fourth (a ':' in the descriptor arms the reference's token state, and a blank
//     behind it would close a "token" there);
//   * class and size: decimal, 1-9 digits, no leading zero but for "0" (keys are strings: "007" is not "7");
//   * behind the fourth tab: nothing, or tokens (A|number):number separated by single blanks, no blank at the end;
//   * no NUL byte, no '\r', no byte >= 0x80 outside the descriptor; the chunk ends with a newline.
// Anything else refuses the whole chunk, which then adds nothing: the host counts it with the reference-exact parser.  One
// deliberate difference: a line of more than GS_KC_LONG_LINE bytes makes the reference fail; here it counts, and is reported.
//
// No lane walks a line.  A thread owns 16 bytes, a block GS_KC_TILE; newlines, tabs and token candidates before every byte come
// from the block scan of gs_scan.h and gs_launch_scan_blocks over the per-block sums.  With exactly four tabs on every line in front
// of it, the field of a byte is (tabs before it) - 4 * (newlines before it): a line that breaks the rule is found at its own fifth
// tab or its own newline, and later lines no longer matter.  A token is the first counted one of its line iff the candidates in
// front of it equal those in front of the line's fourth tab (line_c4).  The lane behind a delimiter parses the one field or token
// that starts there: at most 22 bytes, out of the LDS copy of the block and 32 bytes behind it.
//   kc_count_kernel   per block: newlines, tabs, candidates                                  1 read of the text
//   kc_check_kernel   the grammar; per line: newline offset, line_c4, class                  1 read
//   kc_accum_kernel   (skipped if refused) tokens -> LDS table of GS_KC_LDS_SLOTS keys per workgroup of GS_KC_GROUP blocks,
//                     flushed once: one global atomic per workgroup, key and non-zero counter    1 read
//   kc_commit_kernel  per slot of the global table: the chunk's sums join the rows, or (refused, table full) its claims go
//   kc_finish_kernel  one thread: totals, the chunk's report, status words for the next chunk
// The table: open addressing over uint32 keys.  A chunk first CLAIMS slots for new keys (key set, row not yet present) and adds
// into `delta`; only the commit makes rows, so a chunk that overflows the table leaves it as it was.  Removing claims cannot break
// a probe chain of an older key: claims only ever took slots that were free when the older keys went in.
// Sizing of the privatisation (in a typical file "0" takes half of all tokens, a handful of tax ids the rest): a workgroup sees
// 32 KiB, some 300 lines of 100 bytes with 2-3 tokens each, ~800 tokens and ~10 distinct keys -> ~25 global atomics per
// workgroup, 0.03 per token; without the LDS table the "0" row alone would take one atomic per two tokens on ONE address.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gs_launch.h"
#include "gs_params.h"
#include "gs_scan.h"

#define KC_BLOCK GS_SCAN_BLOCK
static_assert(KC_BLOCK * 16 == GS_KC_TILE, "a thread owns 16 bytes of its block");
#define KC_TEXT0 16                               // where the block's first byte lies in its LDS copy: the byte in front of it at 15
#define KC_TEXT_LDS (KC_TEXT0 + GS_KC_TILE + 32)  // and 32 bytes behind it

struct KcLane {
    uint32_t L, g, c;            // newlines, tabs, candidates in front of the thread's first byte
    uint32_t nlm, tabm, candm;   // bit i: byte i is a newline / a tab / a candidate
};

__device__ __forceinline__ void kc_masks(const uint32_t w[4], uint32_t prev, uint32_t &nlm, uint32_t &tabm, uint32_t &candm) {
    nlm = tabm = candm = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        nlm |= (uint32_t)(b == '\n') << i;
        tabm |= (uint32_t)(b == '\t') << i;
        candm |= (uint32_t)((prev == ' ' || prev == '\t') && b - '0' < 10u) << i;
        prev = b;
    }
}

__global__ __launch_bounds__(KC_BLOCK) void kc_count_kernel(GsKrakenCountParams P) {
    __shared__ uint32_t s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = ((size_t)blockIdx.x * KC_BLOCK + threadIdx.x) * 16;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t nlm, tabm, candm;
    kc_masks(w, base ? P.text[base - 1] : '\n', nlm, tabm, candm);
    if (nlm) atomicAdd(&s_cnt[0], (uint32_t)__popc(nlm));
    if (tabm) atomicAdd(&s_cnt[1], (uint32_t)__popc(tabm));
    if (candm) atomicAdd(&s_cnt[2], (uint32_t)__popc(candm));
    __syncthreads();
    if (threadIdx.x == 0) {
        P.tile_lt[blockIdx.x] = (u64)s_cnt[0] | (u64)s_cnt[1] << 32;
        P.tile_c[blockIdx.x] = s_cnt[2];
    }
}

// block `tile` into s_text; what lies in front of the thread's 16 bytes.  Every thread of the block arrives; s_wave: 2 * KC_BLOCK / 64
// words.  The caller passes a barrier before the next call.
__device__ __forceinline__ KcLane kc_front(const GsKrakenCountParams &P, int64_t tile, uint8_t *s_text, u64 *s_wave) {
    const size_t tile0 = (size_t)tile * GS_KC_TILE;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + tile0 + threadIdx.x * 16);
    *reinterpret_cast<uint4 *>(s_text + KC_TEXT0 + threadIdx.x * 16) = v;
    if (threadIdx.x < 2)  // (the text's buffer ends 64 zero bytes behind its last block)
        *reinterpret_cast<uint4 *>(s_text + KC_TEXT0 + GS_KC_TILE + threadIdx.x * 16) =
            *reinterpret_cast<const uint4 *>(P.text + tile0 + GS_KC_TILE + threadIdx.x * 16);
    if (threadIdx.x == 2) s_text[KC_TEXT0 - 1] = tile ? P.text[tile0 - 1] : '\n';
    __syncthreads();
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    KcLane k;
    kc_masks(w, s_text[KC_TEXT0 + threadIdx.x * 16 - 1], k.nlm, k.tabm, k.candm);
    u64 total;
    const u64 lt = gs_block_scan((u64)__popc(k.nlm) | (u64)__popc(k.tabm) << 32, s_wave, &total) + P.tile_lt[tile];
    const u64 c = gs_block_scan((u64)__popc(k.candm), s_wave + KC_BLOCK / 64, &total) + P.tile_c[tile];
    k.L = (uint32_t)lt;
    k.g = (uint32_t)(lt >> 32);
    k.c = (uint32_t)c;
    return k;
}

// a number of the grammar at s[i]: 1-9 digits, no leading zero but for "0"; i: behind its digits (at most 10 are read)
__device__ __forceinline__ bool kc_number(const uint8_t *s, int &i, uint32_t &val) {
    const uint8_t first = s[i];
    uint32_t v = 0;
    int n = 0;
    for (; n < 10; n++, i++) {
        const uint32_t d = (uint32_t)s[i] - '0';
        if (d > 9u) break;
        v = v * 10u + d;
    }
    val = v;
    return n >= 1 && n <= 9 && !(first == '0' && n > 1);
}

// the token at s[i]: (A|number):number and a blank or a newline behind it
__device__ __forceinline__ bool kc_token(const uint8_t *s, int i, bool &is_a, uint32_t &taxid, uint32_t &count) {
    is_a = s[i] == 'A';
    taxid = 0;
    if (is_a)
        i++;
    else if (!kc_number(s, i, taxid))
        return false;
    if (s[i] != ':') return false;
    i++;
    if (!kc_number(s, i, count)) return false;
    return s[i] == ' ' || s[i] == '\n';
}

__device__ __forceinline__ void kc_bad(const GsKrakenCountParams &P, uint32_t line) { atomicMin(&P.status[GS_KC_BAD_LINE], line); }

__global__ __launch_bounds__(KC_BLOCK) void kc_check_kernel(GsKrakenCountParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[KC_TEXT_LDS];
    __shared__ u64 s_wave[2 * KC_BLOCK / 64];
    const KcLane k = kc_front(P, blockIdx.x, s_text, s_wave);
    const uint8_t *s = s_text + KC_TEXT0 + threadIdx.x * 16;
    const int64_t base = ((int64_t)blockIdx.x * KC_BLOCK + threadIdx.x) * 16;
    uint32_t L = k.L, g = k.g, c = k.c;
    for (int i = 0; i < 16 && base + i < P.n_bytes; i++) {
        const uint8_t b = s[i];
        const int64_t r = (int64_t)g - 4 * (int64_t)L;  // the field of the byte: tabs in front of it on its line
        if (k.nlm >> i & 1) {
            if (s[i - 1] == '\n') {  // (the byte in front of the chunk counts as a newline)
                atomicMin(&P.status[GS_KC_EMPTY_LINE], L);
                atomicMin(&P.status[GS_KC_EMPTY_OFF], (uint32_t)(base + i));
            } else if (r != 4) {
                kc_bad(P, L);
            }
            if ((int64_t)L < P.line_cap) P.line_end[L] = (uint32_t)(base + i);
            L++;
        } else if (k.tabm >> i & 1) {
            uint32_t val;
            int j = i + 1;
            if (r == 1 || r == 2) {  // the class, the read size
                if (!kc_number(s, j, val) || s[j] != '\t') kc_bad(P, L);
                if (r == 1 && (int64_t)L < P.line_cap) P.line_key[L] = val;
            } else if (r == 3) {
                bool is_a;
                uint32_t count;
                if ((int64_t)L < P.line_cap) P.line_c4[L] = c;
                if (s[j] != '\n' && !kc_token(s, j, is_a, val, count)) kc_bad(P, L);
            } else if (r != 0) {
                kc_bad(P, L);
            }
            g++;
        } else if (b == ' ') {
            bool is_a;
            uint32_t val, count;
            if (r != 4 || !kc_token(s, i + 1, is_a, val, count)) kc_bad(P, L);
        } else if (b == 0 || b == '\r' || (b >= 0x80 && r != 1)) {
            kc_bad(P, L);
        }
        if (base + i == P.n_bytes - 1 && b != '\n') kc_bad(P, L);
        c += k.candm >> i & 1;
    }
}

__device__ __forceinline__ uint32_t kc_hash(uint32_t key) { return key * 0x9e3779b1u; }

// the slot of `key` in the global table, claimed if the key is new; GS_KC_EMPTY: no room
__device__ uint32_t kc_global_slot(const GsKrakenCountParams &P, uint32_t key, uint32_t *n_atomics) {
    uint32_t h = kc_hash(key) >> (32 - P.slot_bits);
    for (uint32_t step = 0; step < P.n_slots; step++, h = (h + 1) & (P.n_slots - 1)) {
        uint32_t k = __hip_atomic_load(&P.keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == GS_KC_EMPTY) {
            k = atomicCAS(&P.keys[h], GS_KC_EMPTY, key);
            ++*n_atomics;
            if (k == GS_KC_EMPTY) {
                ++*n_atomics;
                if (atomicAdd(&P.n_keys[1], 1u) >= P.max_keys) atomicOr(&P.status[GS_KC_FULL], 1u);
                return h;
            }
        }
        if (k == key) return h;
    }
    atomicOr(&P.status[GS_KC_FULL], 1u);
    return GS_KC_EMPTY;
}

__device__ __forceinline__ void kc_global_add(const GsKrakenCountParams &P, uint32_t slot, int which, u64 n, uint32_t *n_atomics) {
    if (slot == GS_KC_EMPTY || n == 0) return;
    atomicAdd(&P.delta[(size_t)slot * 3 + which], n);
    ++*n_atomics;
}

struct KcTable {
    uint32_t *key;  // GS_KC_LDS_SLOTS
    u64 *cnt;       // 3 per slot
};

// the workgroup's slot of `key`, or -1
__device__ __forceinline__ int kc_lds_slot(const KcTable &t, uint32_t key) {
    uint32_t h = kc_hash(key) >> 23;
    static_assert(GS_KC_LDS_SLOTS == 512, "kc_lds_slot takes the top 9 bits of the hash");
    for (int step = 0; step < GS_KC_LDS_PROBES; step++, h = (h + 1) & (GS_KC_LDS_SLOTS - 1)) {
        uint32_t k = *(volatile uint32_t *)&t.key[h];
        if (k == GS_KC_EMPTY) k = atomicCAS(&t.key[h], GS_KC_EMPTY, key);
        if (k == GS_KC_EMPTY || k == key) return (int)h;
    }
    return -1;
}

// row[key].counter[which] += n; the row comes into being even where n is 0
__device__ __forceinline__ void kc_add(const GsKrakenCountParams &P, const KcTable &t, uint32_t key, int which, u64 n, uint32_t *n_atomics,
                                       uint32_t *n_direct) {
    const int slot = kc_lds_slot(t, key);
    if (slot >= 0) {
        if (n) atomicAdd(&t.cnt[slot * 3 + which], n);
        return;
    }
    ++*n_direct;
    kc_global_add(P, kc_global_slot(P, key, n_atomics), which, n, n_atomics);
}

__global__ __launch_bounds__(KC_BLOCK) void kc_accum_kernel(GsKrakenCountParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_text[KC_TEXT_LDS];
    __shared__ u64 s_wave[2 * KC_BLOCK / 64];
    __shared__ uint32_t s_key[GS_KC_LDS_SLOTS];
    __shared__ u64 s_cnt[GS_KC_LDS_SLOTS * 3];
    __shared__ uint32_t s_tot[6];  // lines, counted tokens, 'A' tokens, long lines; global atomics, tokens straight to the global table
    const uint32_t bad = P.status[GS_KC_BAD_LINE], first_empty = P.status[GS_KC_EMPTY_LINE];
    if (bad < first_empty) return;  // refused: the chunk adds nothing
    for (int i = threadIdx.x; i < GS_KC_LDS_SLOTS; i += KC_BLOCK) {
        s_key[i] = GS_KC_EMPTY;
        s_cnt[3 * i] = s_cnt[3 * i + 1] = s_cnt[3 * i + 2] = 0;
    }
    if (threadIdx.x < 6) s_tot[threadIdx.x] = 0;
    const KcTable t{s_key, s_cnt};
    uint32_t n_lines = 0, n_counted = 0, n_a = 0, n_long = 0, n_atomics = 0, n_direct = 0;
    const int64_t tile_end = (int64_t)(blockIdx.x + 1) * GS_KC_GROUP < P.n_tiles ? (int64_t)(blockIdx.x + 1) * GS_KC_GROUP : P.n_tiles;
    for (int64_t tile = (int64_t)blockIdx.x * GS_KC_GROUP; tile < tile_end; tile++) {
        const KcLane k = kc_front(P, tile, s_text, s_wave);  // (its barrier also stands between the table's initialisation and its use)
        const uint8_t *s = s_text + KC_TEXT0 + threadIdx.x * 16;
        const int64_t base = (tile * KC_BLOCK + threadIdx.x) * 16;
        uint32_t L = k.L, c = k.c;
        uint32_t g = k.g;
        for (int i = 0; i < 16 && base + i < P.n_bytes && L < first_empty; i++) {
            const bool tab4 = (k.tabm >> i & 1) && g - 4 * L == 3;
            g += k.tabm >> i & 1;
            if (k.nlm >> i & 1) {
                const uint32_t start = L ? P.line_end[L - 1] + 1u : 0u;
                n_lines++;
                n_long += (uint32_t)(base + i) - start + 1u > GS_KC_LONG_LINE;
                L++;
            } else if ((tab4 && s[i + 1] != '\n') || s[i] == ' ') {
                bool is_a;
                uint32_t taxid, count;
                kc_token(s, i + 1, is_a, taxid, count);
                if (is_a) {
                    n_a++;
                } else {
                    n_counted++;
                    kc_add(P, t, taxid, GS_KC_KMERS, count, &n_atomics, &n_direct);
                    // (the candidate of this token lies behind byte i: c counts those in front of it, as line_c4 does for the tab)
                    if (c + (k.candm >> i & 1) == P.line_c4[L]) {  // the first counted token of its line
                        const uint32_t cls = P.line_key[L];
                        kc_add(P, t, cls, GS_KC_READS, 1, &n_atomics, &n_direct);
                        if (cls == taxid) kc_add(P, t, cls, GS_KC_KIMR, count, &n_atomics, &n_direct);
                    }
                }
            }
            c += k.candm >> i & 1;
        }
        __syncthreads();
    }
    // the flush: one global atomic per key and non-zero counter of the workgroup
    for (int i = threadIdx.x; i < GS_KC_LDS_SLOTS; i += KC_BLOCK) {
        if (s_key[i] == GS_KC_EMPTY) continue;
        const uint32_t slot = kc_global_slot(P, s_key[i], &n_atomics);
        for (int which = 0; which < 3; which++) kc_global_add(P, slot, which, s_cnt[3 * i + which], &n_atomics);
    }
    if (n_lines) atomicAdd(&s_tot[0], n_lines);
    if (n_counted) atomicAdd(&s_tot[1], n_counted);
    if (n_a) atomicAdd(&s_tot[2], n_a);
    if (n_long) atomicAdd(&s_tot[3], n_long);
    if (n_atomics) atomicAdd(&s_tot[4], n_atomics);
    if (n_direct) atomicAdd(&s_tot[5], n_direct);
    __syncthreads();
    if (threadIdx.x < 6 && s_tot[threadIdx.x]) atomicAdd(&P.chunk_tot[threadIdx.x], (u64)s_tot[threadIdx.x]);
}

__device__ __forceinline__ uint32_t kc_refused(const GsKrakenCountParams &P) {
    if (P.status[GS_KC_BAD_LINE] < P.status[GS_KC_EMPTY_LINE]) return 1;
    return P.status[GS_KC_FULL] ? 2 : 0;
}

__global__ __launch_bounds__(256) void kc_commit_kernel(GsKrakenCountParams P) {
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= P.n_slots || P.keys[slot] == GS_KC_EMPTY) return;
    const bool ok = kc_refused(P) == 0;
    if (!P.present[slot]) {
        if (ok)
            P.present[slot] = 1;
        else
            P.keys[slot] = GS_KC_EMPTY;
    }
    for (int which = 0; which < 3; which++) {
        const u64 d = P.delta[(size_t)slot * 3 + which];
        if (d == 0) continue;
        if (ok) P.acc[(size_t)slot * 3 + which] += d;
        P.delta[(size_t)slot * 3 + which] = 0;
    }
}

__global__ void kc_finish_kernel(GsKrakenCountParams P) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t refused = kc_refused(P);
    u64 *R = P.result;
    R[GS_KC_R_REFUSED] = refused;
    R[GS_KC_R_BAD_LINE] = refused == 1 ? (u64)P.status[GS_KC_BAD_LINE] : ~0ULL;
    R[GS_KC_R_EMPTY_OFF] = refused == 0 && P.status[GS_KC_EMPTY_OFF] != GS_KC_EMPTY ? (u64)P.status[GS_KC_EMPTY_OFF] : ~0ULL;
    if (refused == 0)
        P.n_keys[0] = P.n_keys[1];
    else
        P.n_keys[1] = P.n_keys[0];
    R[GS_KC_R_ROWS] = P.n_keys[0];
    for (int i = 0; i < 4; i++) {
        const u64 v = refused == 0 ? P.chunk_tot[i] : 0;
        R[GS_KC_R_CHUNK + i] = v;
        P.run_tot[i] += v;
        R[GS_KC_R_RUN + i] = P.run_tot[i];
        P.chunk_tot[i] = 0;
    }
    if (refused == 0) {
        P.counters[0] += P.chunk_tot[4];
        P.counters[1] += P.chunk_tot[5];
    }
    P.chunk_tot[4] = P.chunk_tot[5] = 0;
    P.status[GS_KC_BAD_LINE] = P.status[GS_KC_EMPTY_LINE] = P.status[GS_KC_EMPTY_OFF] = GS_KC_EMPTY;
    P.status[GS_KC_FULL] = 0;
}

__global__ __launch_bounds__(256) void kc_reset_kernel(GsKrakenCountParams P) {
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    if (slot < P.n_slots) {
        P.keys[slot] = GS_KC_EMPTY;
        P.present[slot] = 0;
        for (int which = 0; which < 3; which++) P.acc[(size_t)slot * 3 + which] = P.delta[(size_t)slot * 3 + which] = 0;
    }
    if (slot == 0) {
        for (int i = 0; i < 6; i++) P.chunk_tot[i] = 0;
        for (int i = 0; i < 4; i++) P.run_tot[i] = 0;
        P.counters[0] = P.counters[1] = 0;
        P.n_keys[0] = P.n_keys[1] = 0;
        P.status[GS_KC_BAD_LINE] = P.status[GS_KC_EMPTY_LINE] = P.status[GS_KC_EMPTY_OFF] = GS_KC_EMPTY;
        P.status[GS_KC_FULL] = 0;
    }
}

// one chunk: the grammar, then -- gated on the device by what the check left in P.status -- its tokens into the table; P.result
// says what became of it.  P.n_bytes > 0.
extern "C" hipError_t gs_launch_krakencount(const GsKrakenCountParams *P, hipStream_t stream) {
    const unsigned n_tiles = (unsigned)P->n_tiles;
    hipLaunchKernelGGL(kc_count_kernel, dim3(n_tiles), dim3(KC_BLOCK), 0, stream, *P);
    hipError_t e = gs_launch_scan_blocks(P->tile_lt, P->n_tiles, P->scan_tot, stream);
    if (e == hipSuccess) e = gs_launch_scan_blocks(P->tile_c, P->n_tiles, P->scan_tot + 1, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kc_check_kernel, dim3(n_tiles), dim3(KC_BLOCK), 0, stream, *P);
    hipLaunchKernelGGL(kc_accum_kernel, dim3((n_tiles + GS_KC_GROUP - 1) / GS_KC_GROUP), dim3(KC_BLOCK), 0, stream, *P);
    hipLaunchKernelGGL(kc_commit_kernel, dim3((P->n_slots + 255) / 256), dim3(256), 0, stream, *P);
    hipLaunchKernelGGL(kc_finish_kernel, dim3(1), dim3(64), 0, stream, *P);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_krakencount_reset(const GsKrakenCountParams *P, hipStream_t stream) {
    hipLaunchKernelGGL(kc_reset_kernel, dim3((P->n_slots + 255) / 256), dim3(256), 0, stream, *P);
    return hipGetLastError();
}
