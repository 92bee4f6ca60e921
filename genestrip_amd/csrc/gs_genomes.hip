// gs_genomes.hip -- genome FASTA text to build regions on the device (the front of gs_dbsize / gs_dbbuild / gs_dbupdate / gs_dbquality).
//
// The reference walks a genome collection with AbstractFastaReader.readFasta (C/fasta/AbstractFastaReader.java:97-130) over
// BufferedLineReader.nextLine (B/io/BufferedLineReader.java:160-182), one thread, up to four times per build; what the store
// readers make of a data line is AbstractStoreFastaReader.dataLine (C/refseq/AbstractStoreFastaReader.java:87-114):
//   * a line runs up to and including its '\n'; the last line of a stream may lack one;
//   * a line whose first byte is '>' is a header line: it ends the region before it and starts the next; every other line is a
//     data line of the current region; data lines in front of the first header belong to no region;
//   * of a data line the whole trailing run of '\n' / '\r' is stripped (the while at :95), every other byte is a base of the
//     region, a '\r' with a byte of the same line behind its run included; an empty line gives nothing and is no error;
//   * a NUL byte is dropped by nextLine before anything looks at the line: such a chunk is REFUSED here (the host parser's case).
// Which regions count, and for which node, stays the host's decision: the scan hands it the header lines, the gather takes one
// keep flag per record back and writes the bases of the kept records alone, as (seq, off) of the region stage.
//
// No lane walks a line or a record (an unwrapped chromosome is ONE line).  A thread owns 16 bytes of text, a block GS_GN_TILE;
// header lines, newlines and CONTENT bytes (bytes that are no part of their line's trailing terminator run) in front of every
// byte come from the block scan of gs_scan.h and gs_launch_scan_blocks over the per-tile sums.  With C(p) = content bytes in
// front of byte p: the content of a line is a prefix of it, so a record's bases are the content indices
// [C(behind its header line), C(next header)), a byte is a base of record r iff its content index is not below the first of the
// two (base_start[r]; header bytes lie below it), and it goes to off[j] + C(p) - base_start[r].  The gather is therefore cut by
// TEXT: 16 source bytes per lane, and 16 content bytes of one record -- nearly every lane of a data line -- are one 16-byte store
// (global stores need no alignment on gfx950; the destination is aligned only by chance).  Tiles none of whose records is kept
// return before they read their text.
// Whether a '\r' is content needs the byte behind its run: a look-ahead of at most GS_GN_CR_CAP bytes.  A run of more than GS_GN_CR_CAP
// '\r' refuses the chunk, so the look-ahead stays linear in the worst case (GS_GN_CR_CAP + 1 reads per '\r').
// The text lies in the handle's own buffer with GS_GN_PAD bytes of '\n' behind it: no load of these kernels needs a bounds check, and
// a look-ahead that runs off the end of the stream finds the terminator the reference's loop finds there (the bare '\r' at the
// end of a stream IS stripped: :95 does not ask for a '\n').
//
//   gn_count_kernel    per tile: header lines, newlines, content bytes; first NUL, first over-long '\r' run       1 read of the text
//   (gs_launch_scan_blocks x 2)
//   gn_lines_kernel    per newline: its offset and C behind it; per header line: its offset and its line number    1 read
//   gn_records_kernel  per record: header length (scanned inside blocks of 256 records), base_start, bases
//   gn_hdr_off_kernel  per record: + its block's prefix -> hdr_off
//   gn_maxline_kernel  per line in front of the cut: its length with its newline -> the chunk's longest; the cut itself
//   gn_headers_kernel  one wave per record: its header line -> the compact header buffer (headers are short; the host reads them)
//   gn_select_kernel   per record: kept? its bases; scanned inside blocks          gn_offsets_kernel  + block prefix -> sel, off
//   gn_gather_kernel   per tile that holds bases of a kept record: the bases                               <= 1 read, 1 write of the kept
// Occupancy / LDS (256 threads, 16 bytes each, no arrays indexed at run time): every kernel stays far below 64 VGPRs and uses at
// most 32 bytes of LDS (the wave sums of the block scan; gn_count_kernel: the tile's three counters), so 8 waves per SIMD.
// A record ENDS inside a chunk when a later header line exists, or always when the chunk is the stream's last; the cut (consumed
// bytes) is the start of the last header line otherwise (without any header line: behind the last newline -- those lines belong
// to no region or to one the caller has not kept whole, see gs_genomes_scan).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gs_launch.h"
#include "gs_params.h"
#include "gs_scan.h"

#define GN_BLOCK GS_SCAN_BLOCK
static_assert(GN_BLOCK * 16 == GS_GN_TILE, "a thread owns 16 bytes of its tile");
#define GN_KEPT (1ULL << 40)  // gn_select: kept records above bit 40, their bases below (a chunk holds at most 2^30 bytes)
static_assert(GS_GN_MAX_RECORDS - 1ULL <= (~0ULL >> 40),
              "the caller refuses chunks of GS_GN_MAX_RECORDS header lines and more: the kept count has the 24 bits above bit 40");
#define GN_LOW (GN_KEPT - 1)

struct GnLane {
    uint32_t hdrm, nlm, contm;  // bit i: byte i opens a header line / is a newline / is content (bytes behind the text: none)
    uint32_t nul, crbad;        // first NUL byte / first '\r' that opens a run of more than GS_GN_CR_CAP (offsets; ~0: none)
};

// is the '\r' at p content?  Only if the byte behind its run of '\r' is no '\n' (behind the text lie '\n's).  run_start: no '\r'
// in front of it; such a one also finds out whether its run is longer than the cap
__device__ __forceinline__ bool gn_cr_kept(const uint8_t *text, size_t p, bool run_start, uint32_t &crbad) {
    size_t q = p + 1;
    while (q - p <= GS_GN_CR_CAP && text[q] == '\r') q++;
    if (run_start && q - p > GS_GN_CR_CAP) crbad = min(crbad, (uint32_t)p);
    return text[q] != '\n';  // (past the cap: the chunk is refused by the run's first byte, the answer is not used)
}

__device__ __forceinline__ GnLane gn_lane(const GsGenomesParams &P, size_t base) {
    GnLane k;
    k.hdrm = k.nlm = k.contm = 0;
    k.nul = k.crbad = 0xffffffffu;
    const uint4 v = *reinterpret_cast<const uint4 *>(P.text + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t prev = base ? P.text[base - 1] : '\n';
    const int64_t left = P.n_bytes - (int64_t)base;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        if (i < left) {
            bool cont = b != '\n';
            if (b == '\r') cont = gn_cr_kept(P.text, base + i, prev != '\r', k.crbad);
            if (b == 0) k.nul = min(k.nul, (uint32_t)(base + i));
            k.nlm |= (uint32_t)(b == '\n') << i;
            k.hdrm |= (uint32_t)(b == '>' && prev == '\n') << i;
            k.contm |= (uint32_t)cont << i;
        }
        prev = b;
    }
    return k;
}

// where the records that end inside the chunk end (see the head of the file)
__device__ __forceinline__ uint32_t gn_cut(const GsGenomesParams &P) {
    if (P.last) return (uint32_t)P.n_bytes;
    if (P.n_hdr > 0) return P.rec_start[P.n_hdr - 1];
    return P.n_nl > 0 ? P.nl[P.n_nl - 1] + 1u : 0u;
}

__global__ __launch_bounds__(GN_BLOCK) void gn_count_kernel(GsGenomesParams P) {
    __shared__ uint32_t s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const GnLane k = gn_lane(P, ((size_t)blockIdx.x * GN_BLOCK + threadIdx.x) * 16);
    if (k.hdrm) atomicAdd(&s_cnt[0], (uint32_t)__popc(k.hdrm));
    if (k.nlm) atomicAdd(&s_cnt[1], (uint32_t)__popc(k.nlm));
    if (k.contm) atomicAdd(&s_cnt[2], (uint32_t)__popc(k.contm));
    if (k.nul != 0xffffffffu) atomicMin(&P.status[GS_GN_NUL], k.nul);
    if (k.crbad != 0xffffffffu) atomicMin(&P.status[GS_GN_CR], k.crbad);
    __syncthreads();
    if (threadIdx.x == 0) {
        P.tile_hl[blockIdx.x] = (u64)s_cnt[1] | (u64)s_cnt[0] << 32;
        P.tile_c[blockIdx.x] = s_cnt[2];
    }
}

// header lines (bits 40..), newlines (20..39) and content bytes (0..19) of the tile in front of the thread's bytes
#define GN_PACK(k) ((u64)__popc((k).hdrm) << 40 | (u64)__popc((k).nlm) << 20 | (u64)__popc((k).contm))

__global__ __launch_bounds__(GN_BLOCK) void gn_lines_kernel(GsGenomesParams P) {
    __shared__ u64 s_wave[GN_BLOCK / 64];
    const size_t base = ((size_t)blockIdx.x * GN_BLOCK + threadIdx.x) * 16;
    const GnLane k = gn_lane(P, base);
    u64 total;
    const u64 ex = gs_block_scan(GN_PACK(k), s_wave, &total);
    const u64 hl = P.tile_hl[blockIdx.x];
    int64_t R = (int64_t)(hl >> 32) + (int64_t)(ex >> 40), L = (int64_t)(hl & 0xffffffffu) + (int64_t)((ex >> 20) & 0xfffffu);
    uint32_t c = (uint32_t)P.tile_c[blockIdx.x] + (uint32_t)(ex & 0xfffffu);
    if ((k.hdrm | k.nlm) == 0) return;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (k.hdrm >> i & 1) {
            if (R < P.n_hdr) {  // (the counts are those of gn_count_kernel: always)
                P.rec_start[R] = (uint32_t)(base + i);
                P.rec_line[R] = (uint32_t)L;
            }
            R++;
        }
        if (k.nlm >> i & 1) {
            if (L < P.n_nl) {
                P.nl[L] = (uint32_t)(base + i);
                P.cnl[L] = c;
            }
            L++;
        }
        c += k.contm >> i & 1;
    }
}

__global__ __launch_bounds__(GN_BLOCK) void gn_records_kernel(GsGenomesParams P) {
    __shared__ u64 s_wave[GN_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
    u64 hl = 0;
    if (r < P.n_records) {
        const int64_t L = P.rec_line[r];  // its header line; without a newline it is the stream's last line: no bases
        const uint32_t all = (uint32_t)P.tile_c[P.n_tiles];
        const uint32_t b0 = L < P.n_nl ? P.cnl[L] : all;
        const uint32_t b1 = r + 1 < P.n_hdr ? P.cnl[P.rec_line[r + 1] - 1] : all;  // (a header line behind the first follows a newline)
        hl = (L < P.n_nl ? P.nl[L] : (uint32_t)P.n_bytes) - P.rec_start[r];
        P.base_start[r] = b0;
        P.base_cnt[r] = b1 - b0;
    }
    u64 total;
    const u64 ex = gs_block_scan(hl, s_wave, &total);
    if (r < P.n_records) P.hdr_off[r] = ex;
    if (threadIdx.x == 0) P.rec_block[blockIdx.x] = total;
}

__global__ __launch_bounds__(GN_BLOCK) void gn_hdr_off_kernel(GsGenomesParams P) {
    const int64_t r = (int64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
    if (r < P.n_records) P.hdr_off[r] += P.rec_block[blockIdx.x];
    if (r == 0) P.hdr_off[P.n_records] = P.res[GS_GN_R_HDR_BYTES];
}

// lines 0 .. n_nl - 1 end with a newline, line n_nl is what lies behind the last one (a line only at the end of the stream)
__global__ __launch_bounds__(GN_BLOCK) void gn_maxline_kernel(GsGenomesParams P) {
    const int64_t i = (int64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
    const uint32_t cut = gn_cut(P);
    uint32_t len = 0;
    if (i <= P.n_nl) {
        const uint32_t start = i ? P.nl[i - 1] + 1u : 0u, end = i < P.n_nl ? P.nl[i] + 1u : (uint32_t)P.n_bytes;
        if (start < cut) len = end - start;  // (the cut lies at the start of a line; behind the last newline only with `last`)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) len = max(len, (uint32_t)__shfl_xor((int)len, d));
    if ((threadIdx.x & 63) == 0 && len) atomicMax(&P.status[GS_GN_MAXLINE], len);
    if (i == 0) P.res[GS_GN_R_CUT] = cut;
}

__global__ __launch_bounds__(256) void gn_headers_kernel(GsGenomesParams P) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < P.n_records; r += n_waves) {
        const u64 dst = P.hdr_off[r], len = P.hdr_off[r + 1] - dst;
        const size_t src = P.rec_start[r];
        for (u64 j = (u64)lane; j < len; j += 64) P.hdr_out[dst + j] = P.text[src + j];
    }
}

__global__ __launch_bounds__(GN_BLOCK) void gn_select_kernel(GsGenomesParams P) {
    __shared__ u64 s_wave[GN_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
    u64 v = 0;
    if (r < P.n_records && (P.keep == nullptr || P.keep[r] != 0)) v = GN_KEPT | (u64)P.base_cnt[r];
    u64 total;
    const u64 ex = gs_block_scan(v, s_wave, &total);
    if (r < P.n_records) P.sel[r] = ex;
    if (threadIdx.x == 0) P.rec_block[blockIdx.x] = total;
}

__global__ __launch_bounds__(GN_BLOCK) void gn_offsets_kernel(GsGenomesParams P) {
    const int64_t r = (int64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
    if (r < P.n_records) {
        const u64 s = P.sel[r] + P.rec_block[blockIdx.x];
        P.sel[r] = s;
        if (P.keep == nullptr || P.keep[r] != 0) P.off[s >> 40] = s & GN_LOW;
    }
    if (r == 0) {
        const u64 all = P.res[GS_GN_R_KEPT];
        P.sel[P.n_records] = all;
        P.off[all >> 40] = all & GN_LOW;
    }
}

struct GnRec {
    bool kept;
    uint32_t first;  // base_start
    u64 delta;       // destination of content index c: c + delta (mod 2^64)
};
__device__ __forceinline__ GnRec gn_rec(const GsGenomesParams &P, int64_t r) {
    GnRec g;
    g.kept = false;
    g.first = 0;
    g.delta = 0;
    if (r < 0 || r >= P.n_records) return g;  // in front of the first header line; behind the cut
    const u64 s0 = P.sel[r], s1 = P.sel[r + 1];
    g.kept = (s0 >> 40) != (s1 >> 40);
    g.first = P.base_start[r];
    g.delta = (s0 & GN_LOW) - (u64)g.first;
    return g;
}

__global__ __launch_bounds__(GN_BLOCK) void gn_gather_kernel(GsGenomesParams P) {
    __shared__ u64 s_wave[GN_BLOCK / 64];
    // the records with bytes in this tile: the one that reaches into it and those whose header lines it holds
    const int64_t h0 = (int64_t)(P.tile_hl[blockIdx.x] >> 32), h1 = (int64_t)(P.tile_hl[blockIdx.x + 1] >> 32);
    const int64_t ra = std::min<int64_t>(std::max<int64_t>(h0 - 1, 0), P.n_records), rb = std::min<int64_t>(h1, P.n_records);
    if ((P.sel[ra] >> 40) == (P.sel[rb] >> 40)) return;  // none of them is kept (the same for every thread of the block)
    const size_t base = ((size_t)blockIdx.x * GN_BLOCK + threadIdx.x) * 16;
    const GnLane k = gn_lane(P, base);
    u64 total;
    const u64 ex = gs_block_scan(GN_PACK(k), s_wave, &total);
    int64_t r = h0 + (int64_t)(ex >> 40) - 1;
    u64 c = P.tile_c[blockIdx.x] + (ex & 0xfffffu);
    if (k.contm == 0) return;
    GnRec g = gn_rec(P, r);
    if (k.contm == 0xffffu && k.hdrm == 0) {  // 16 bytes of one line: of a kept record's data, or not
        if (g.kept && c >= g.first) {
            uint4 v = *reinterpret_cast<const uint4 *>(P.text + base);
            __builtin_memcpy(P.seq + (c + g.delta), &v, 16);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (k.hdrm >> i & 1) g = gn_rec(P, ++r);
        if (k.contm >> i & 1) {
            if (g.kept && c >= g.first) P.seq[c + g.delta] = P.text[base + i];
            c++;
        }
    }
}

// per-tile counts and their prefixes: tile_hl / tile_c hold n_tiles + 1 entries, the last one the sum; status has been reset
extern "C" hipError_t gs_launch_genomes_count(const GsGenomesParams *P, hipStream_t stream) {
    if (P->n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(gn_count_kernel, dim3((unsigned)P->n_tiles), dim3(GN_BLOCK), 0, stream, *P);
    gs_launch_scan_blocks(P->tile_hl, P->n_tiles, P->tile_hl + P->n_tiles, stream);
    gs_launch_scan_blocks(P->tile_c, P->n_tiles, P->tile_c + P->n_tiles, stream);
    return hipGetLastError();
}

// the caller has read the sums back: n_hdr, n_nl, n_records are set and the per-line and per-record arrays hold them.
// res: GS_GN_R_CUT, GS_GN_R_HDR_BYTES (zeroed by the caller); status[GS_GN_MAXLINE]
extern "C" hipError_t gs_launch_genomes_records(const GsGenomesParams *P, hipStream_t stream) {
    if (P->n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(gn_lines_kernel, dim3((unsigned)P->n_tiles), dim3(GN_BLOCK), 0, stream, *P);
    const int64_t n_blocks = (P->n_records + GN_BLOCK - 1) / GN_BLOCK;
    if (n_blocks > 0) {
        hipLaunchKernelGGL(gn_records_kernel, dim3((unsigned)n_blocks), dim3(GN_BLOCK), 0, stream, *P);
        gs_launch_scan_blocks(P->rec_block, n_blocks, P->res + GS_GN_R_HDR_BYTES, stream);
        hipLaunchKernelGGL(gn_hdr_off_kernel, dim3((unsigned)n_blocks), dim3(GN_BLOCK), 0, stream, *P);
    }
    hipLaunchKernelGGL(gn_maxline_kernel, dim3((unsigned)((P->n_nl + 1 + GN_BLOCK - 1) / GN_BLOCK)), dim3(GN_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_genomes_headers(const GsGenomesParams *P, hipStream_t stream) {
    if (P->n_records > 0)
        hipLaunchKernelGGL(gn_headers_kernel, dim3((unsigned)std::min<int64_t>((P->n_records + 3) / 4, 8192)), dim3(256), 0, stream, *P);
    return hipGetLastError();
}

// keep -> sel[n_records + 1], off[kept + 1], res[GS_GN_R_KEPT] = kept << 40 | bases (n_records > 0)
extern "C" hipError_t gs_launch_genomes_select(const GsGenomesParams *P, hipStream_t stream) {
    const int64_t n_blocks = (P->n_records + GN_BLOCK - 1) / GN_BLOCK;
    if (n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(gn_select_kernel, dim3((unsigned)n_blocks), dim3(GN_BLOCK), 0, stream, *P);
    gs_launch_scan_blocks(P->rec_block, n_blocks, P->res + GS_GN_R_KEPT, stream);
    hipLaunchKernelGGL(gn_offsets_kernel, dim3((unsigned)n_blocks), dim3(GN_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

// the bases of the kept records -> seq (room for the bases of res[GS_GN_R_KEPT]); cut_tiles: the tiles in front of the cut
extern "C" hipError_t gs_launch_genomes_gather(const GsGenomesParams *P, int64_t cut_tiles, hipStream_t stream) {
    if (cut_tiles > 0 && P->n_records > 0) hipLaunchKernelGGL(gn_gather_kernel, dim3((unsigned)cut_tiles), dim3(GN_BLOCK), 0, stream, *P);
    return hipGetLastError();
}
