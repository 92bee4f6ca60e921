// gs_kraken.hip -- the Kraken-style lines of a FASTQ or FASTA chunk as device text (FastqKMerMatcher.java:308-314, :597-611,
// MatcherReadEntry.writeMatchDetails :723-756; what kraken_line of gs_host.cpp prints on the host), behind the segments kernel.
//
// Per read r of the chunk (nl = newline offsets): descriptor = text[d0, d1) with d0 = r ? nl[4r-1] + 1 : 0 and d1 = nl[4r],
// L = nl[4r+1] - d1 - 1 (a '\r' counts), max = L - k + 1.  A FASTA or general FASTQ chunk (P.rec_line != nullptr, the kernels'
// REC instantiation): the descriptor is line rec_line[r], L = off2[r+1] - off2[r], the gathered read.  No line when the read has
// no segment or !(write_all || class >= 0), else
//   'C' | 'U'  TAB  name  TAB  taxid(class) | '0'  TAB  L  TAB  seg ' ' seg ...  '\n'
// name = the descriptor behind its first byte up to the first blank, seg = taxid(code) | '0' (-1) | 'A' (-2)  ':'  count, count = the
// next segment's start - this one's, for the last one max - start.
//
//   kr_size_kernel     per read: bytes of its line (0: none) and of its name; exclusive scan inside blocks of 256 reads, lines wanted.
//                      A read of many segments or a long descriptor is sized by its whole wave.
//   (gs_launch_scan_blocks, gs_rewrite.hip: the prefix over the blocks, 64-bit -- at small k a line is longer than its record)
//   kr_offsets_kernel  per read: + its block's prefix
//   kr_write_kernel    the text.  The lines of 256 consecutive reads are consecutive in the output: a block builds them in a tile of
//                      LDS, one thread per line, and stores the tile with aligned 16-byte stores (the first and the last 16 bytes of
//                      its range, which it shares with its neighbours, byte by byte).  A line of more than KR_BIG_LINE bytes (hundreds
//                      of segments, a name of kilobytes) is written by the whole block straight to the output, the lines in front of
//                      it and behind it through the tile as usual.  Decimal digits are computed.
//
// This file is also compiled for the HOST, by tests/native/kraken_emulate.cpp (tests/test_krakenlines_cpu.py): g++ with a stand-in
// for <hip/hip_runtime.h> in which a block is 256 real threads, under AddressSanitizer.  Keep to the constructs that stand-in knows
// (tests/native/kraken_emulate_hip.h: ballot, shuffles, __syncthreads, atomicAdd on u64, __shared__ arrays inside a kernel) or
// extend it with the kernel; the same holds for what gs_launch.h, gs_params.h and gs_scan.h pull in (gs_wave.h, the wave helpers of the
// match, route, segments, seen and filter units, is not among it and is not written for the stand-in).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gs_launch.h"
#include "gs_params.h"
#include "gs_scan.h"

#define KR_BLOCK GS_SCAN_BLOCK
#define KR_TILE 32768     // bytes of LDS a block stages its lines in (256 lines of 30 .. 120 bytes: one tile)
#define KR_BIG_LINE 512   // a longer line goes the block-wide way
#define KR_WAVE_SEGS 32   // size pass: a read of more segments ...
#define KR_WAVE_DESC 256  // ... or of a longer descriptor is sized by its wave

struct KrRead {
    uint32_t d0, dlen, L;  // descriptor line, bases
    int32_t cl;
    int64_t maxp;
    u64 s0, s1;            // its segments
};
template <bool REC>
__device__ __forceinline__ KrRead kr_read(const GsKrakenParams &P, int64_t r) {
    KrRead g;
    if (REC) {
        const int64_t i = P.rec_line[r];
        g.d0 = i ? P.nl[i - 1] + 1u : 0u;
        g.dlen = P.nl[i] - g.d0;
        g.L = (uint32_t)(P.off2[r + 1] - P.off2[r]);
    } else {
        g.d0 = r ? P.nl[4 * r - 1] + 1u : 0u;
        const uint32_t d1 = P.nl[4 * r];
        g.dlen = d1 - g.d0;
        g.L = P.nl[4 * r + 1] - d1 - 1u;
    }
    g.maxp = (int64_t)g.L - P.k + 1;
    g.cl = P.cls[r];
    g.s0 = P.seg_off[r];
    g.s1 = P.seg_off[r + 1];
    return g;
}
__device__ __forceinline__ bool kr_wanted(const GsKrakenParams &P, const KrRead &g) { return g.s1 > g.s0 && (P.write_all || g.cl >= 0); }

__device__ __forceinline__ uint32_t kr_digits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}
__device__ __forceinline__ uint32_t kr_tax_len(const GsKrakenParams &P, int32_t vi) { return vi >= 0 ? P.tax_off[vi + 1] - P.tax_off[vi] : 1u; }
// positions of segment sg of a read whose segments end at s1 (printed like the reference's int: a '-' cannot happen for segments of
// the device's)
__device__ __forceinline__ int64_t kr_count(const GsKrakenParams &P, u64 sg, u64 s1, int64_t maxp) {
    return (sg + 1 < s1 ? (int64_t)P.seg_start[sg + 1] : maxp) - (int64_t)P.seg_start[sg];
}
__device__ __forceinline__ uint32_t kr_seg_len(const GsKrakenParams &P, u64 sg, u64 s1, int64_t maxp) {
    const int64_t cnt = kr_count(P, sg, s1, maxp);
    return kr_tax_len(P, P.seg_code[sg]) + 1u + (cnt < 0 ? 1u : 0u) + kr_digits((uint32_t)(cnt < 0 ? -cnt : cnt));
}
// the line without its name and its segments: C TAB TAB taxid TAB L TAB ... NL
__device__ __forceinline__ uint32_t kr_frame_len(const GsKrakenParams &P, const KrRead &g) { return 2u + 1u + kr_tax_len(P, g.cl) + 1u + kr_digits(g.L) + 1u + 1u; }

// where the bytes go: the block's tile (positions relative to the tile's first byte, modulo 2^32: a line that starts in front of the
// tile has its first bytes dropped, one that ends behind it its last) or the output itself
struct KrTile {
    typedef uint32_t Pos;
    uint8_t *lds;
    uint32_t len;
    __device__ __forceinline__ void put(uint32_t q, uint8_t b) const {
        if (q < len) lds[q] = b;
    }
};
struct KrOut {
    typedef u64 Pos;
    uint8_t *out;
    __device__ __forceinline__ void put(u64 q, uint8_t b) const { out[q] = b; }
};

template <class S>
__device__ __forceinline__ typename S::Pos kr_put_uint(const S &s, typename S::Pos pos, uint32_t v) {
    const uint32_t d = kr_digits(v);
    for (uint32_t i = d; i-- > 0;) {
        s.put(pos + i, (uint8_t)('0' + v % 10u));
        v /= 10u;
    }
    return pos + d;
}
template <class S>
__device__ __forceinline__ typename S::Pos kr_put_tax(const S &s, typename S::Pos pos, const GsKrakenParams &P, int32_t vi, uint8_t none) {
    if (vi < 0) {
        s.put(pos, none);
        return pos + 1;
    }
    const uint32_t a = P.tax_off[vi], b = P.tax_off[vi + 1];
    for (uint32_t j = a; j < b; j++) s.put(pos + (j - a), P.tax_bytes[j]);
    return pos + (b - a);
}
template <class S>
__device__ __forceinline__ typename S::Pos kr_put_seg(const S &s, typename S::Pos pos, const GsKrakenParams &P, u64 sg, u64 s1, int64_t maxp) {
    const int32_t code = P.seg_code[sg];
    pos = kr_put_tax(s, pos, P, code, code == -2 ? 'A' : '0');
    s.put(pos++, ':');
    const int64_t cnt = kr_count(P, sg, s1, maxp);
    if (cnt < 0) s.put(pos++, '-');
    return kr_put_uint(s, pos, (uint32_t)(cnt < 0 ? -cnt : cnt));
}
// what stands between the name and the segments: TAB taxid TAB L TAB
template <class S>
__device__ __forceinline__ typename S::Pos kr_put_middle(const S &s, typename S::Pos pos, const GsKrakenParams &P, const KrRead &g) {
    s.put(pos++, '\t');
    pos = kr_put_tax(s, pos, P, g.cl, '0');
    s.put(pos++, '\t');
    pos = kr_put_uint(s, pos, g.L);
    s.put(pos++, '\t');
    return pos;
}
// a whole line by one thread
template <class S>
__device__ __forceinline__ void kr_put_line(const S &s, typename S::Pos pos, const GsKrakenParams &P, const KrRead &g, uint32_t name_len) {
    s.put(pos++, g.cl >= 0 ? 'C' : 'U');
    s.put(pos++, '\t');
    for (uint32_t j = 0; j < name_len; j++) s.put(pos + j, P.text[(size_t)g.d0 + 1 + j]);
    pos = kr_put_middle(s, pos + name_len, P, g);
    for (u64 sg = g.s0; sg < g.s1; sg++) {
        if (sg > g.s0) s.put(pos++, ' ');
        pos = kr_put_seg(s, pos, P, sg, g.s1, g.maxp);
    }
    s.put(pos, '\n');
}

template <bool REC>
__global__ __launch_bounds__(KR_BLOCK) void kr_size_kernel(GsKrakenParams P) {
    __shared__ u64 s_wave[KR_BLOCK / 64];
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
    u64 sz = 0;
    uint32_t name_len = 0;
    bool by_wave = false;
    if (r < P.n_reads) {
        const KrRead g = kr_read<REC>(P, r);
        if (kr_wanted(P, g)) {
            sz = kr_frame_len(P, g);
            by_wave = g.s1 - g.s0 > KR_WAVE_SEGS || g.dlen > KR_WAVE_DESC;
            if (!by_wave) {
                uint32_t j = 1;
                while (j < g.dlen && P.text[(size_t)g.d0 + j] != ' ') j++;
                name_len = g.dlen > 1 ? j - 1 : 0;
                u64 segs = g.s1 - g.s0 - 1;  // the blanks between them
                for (u64 sg = g.s0; sg < g.s1; sg++) segs += kr_seg_len(P, sg, g.s1, g.maxp);
                sz += name_len + segs;
            }
        }
    }
    for (u64 todo = __ballot(by_wave); todo; todo &= todo - 1) {  // the whole wave on one read after the other
        const int src = __ffsll((long long)todo) - 1;
        const KrRead g = kr_read<REC>(P, r - lane + src);
        uint32_t nm = g.dlen > 1 ? g.dlen - 1 : 0;
        for (uint32_t base = 1; base < g.dlen; base += 64) {
            const uint32_t j = base + (uint32_t)lane;
            const u64 hit = __ballot(j < g.dlen && P.text[(size_t)g.d0 + j] == ' ');
            if (hit) {
                nm = base + (uint32_t)(__ffsll((long long)hit) - 1) - 1;
                break;
            }
        }
        u64 segs = 0;
        for (u64 sg = g.s0 + (u64)lane; sg < g.s1; sg += 64) segs += kr_seg_len(P, sg, g.s1, g.maxp);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) segs += __shfl_xor(segs, d);
        if (lane == src) {
            name_len = nm;
            sz += nm + segs + (g.s1 - g.s0 - 1);
        }
    }
    const u64 wanted = __ballot(sz != 0);
    if (lane == 0 && wanted) atomicAdd(&P.totals[1], (u64)__popcll(wanted));
    u64 total;
    const u64 ex = gs_block_scan(sz, s_wave, &total);
    if (r < P.n_reads) {
        P.rec_out[r] = ex;
        P.name_len[r] = name_len;
    }
    if (threadIdx.x == 0) P.rec_block[blockIdx.x] = total;
}

__global__ __launch_bounds__(KR_BLOCK) void kr_offsets_kernel(GsKrakenParams P) {
    const int64_t r = (int64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
    if (r < P.n_reads) P.rec_out[r] += P.rec_block[blockIdx.x];
    if (r == 0) P.rec_out[P.n_reads] = P.totals[0];
}

// The lines that lie in the output range [lo, hi) -- whole lines, each of at most KR_BIG_LINE bytes, `mine`: this thread's line starts
// at `at` and is one of them -- through the tile, KR_TILE bytes from an aligned position at a time.  Every thread of the block arrives.
__device__ __forceinline__ void kr_range(const GsKrakenParams &P, uint8_t *s_tile, u64 lo, u64 hi, bool mine, u64 at, u64 sz, const KrRead &g,
                                         uint32_t name_len) {
    if (lo >= hi) return;
    for (u64 w0 = lo & ~(u64)15; w0 < hi; w0 += KR_TILE) {
        const uint32_t wlen = (uint32_t)std::min<u64>(KR_TILE, hi - w0);
        if (mine && at < w0 + wlen && at + sz > w0) kr_put_line(KrTile{s_tile, wlen}, (uint32_t)(at - w0), P, g, name_len);
        __syncthreads();
        for (uint32_t c = threadIdx.x * 16u; c < wlen; c += KR_BLOCK * 16u) {
            const u64 pos = w0 + c;
            if (pos >= lo && c + 16u <= wlen) {
                *reinterpret_cast<uint4 *>(P.out + pos) = *reinterpret_cast<const uint4 *>(s_tile + c);
            } else {  // the range's first and last 16 bytes: the rest of them is a neighbour's
                for (uint32_t j = 0; j < 16u; j++)
                    if (pos + j >= lo && c + j < wlen) P.out[pos + j] = s_tile[c + j];
            }
        }
        __syncthreads();
    }
}

// one long line by the whole block, straight to the output
template <bool REC>
__device__ __forceinline__ void kr_big_line(const GsKrakenParams &P, u64 *s_wave, int64_t r) {
    const KrRead g = kr_read<REC>(P, r);
    const uint32_t name_len = P.name_len[r];
    const u64 at = P.rec_out[r], end = P.rec_out[r + 1];
    const KrOut s{P.out};
    for (uint32_t j = threadIdx.x; j < name_len; j += KR_BLOCK) P.out[at + 2 + j] = P.text[(size_t)g.d0 + 1 + j];
    if (threadIdx.x == 0) {
        s.put(at, g.cl >= 0 ? 'C' : 'U');
        s.put(at + 1, '\t');
        kr_put_middle(s, at + 2 + name_len, P, g);
        s.put(end - 1, '\n');
    }
    u64 run = at + 2 + name_len + (kr_frame_len(P, g) - 3u);  // (the frame: 2 bytes in front of the name, 1 behind the segments)
    for (u64 c0 = g.s0; c0 < g.s1; c0 += KR_BLOCK) {
        const u64 sg = c0 + threadIdx.x;
        const u64 len = sg < g.s1 ? kr_seg_len(P, sg, g.s1, g.maxp) + (sg > g.s0 ? 1u : 0u) : 0u;
        u64 total;
        u64 pos = run + gs_block_scan(len, s_wave, &total);
        if (sg < g.s1) {
            if (sg > g.s0) s.put(pos++, ' ');
            kr_put_seg(s, pos, P, sg, g.s1, g.maxp);
        }
        run += total;
        __syncthreads();  // (s_wave is free again)
    }
}

template <bool REC>
__global__ __launch_bounds__(KR_BLOCK) void kr_write_kernel(GsKrakenParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[KR_TILE];
    __shared__ u64 s_wave[KR_BLOCK / 64];
    __shared__ u64 s_big[KR_BLOCK / 64];
    const int64_t r0 = (int64_t)blockIdx.x * KR_BLOCK, r = r0 + threadIdx.x;
    const u64 first = P.rec_out[r0], last = P.rec_out[std::min<int64_t>(r0 + KR_BLOCK, P.n_reads)];
    if (first == last) return;  // (the whole block: none of its reads prints a line)
    KrRead g{};
    u64 at = 0, sz = 0;
    uint32_t name_len = 0;
    if (r < P.n_reads) {
        at = P.rec_out[r];
        sz = P.rec_out[r + 1] - at;
        if (sz != 0) {
            g = kr_read<REC>(P, r);
            name_len = P.name_len[r];
        }
    }
    const u64 big = __ballot(sz > KR_BIG_LINE);
    if ((threadIdx.x & 63) == 0) s_big[threadIdx.x >> 6] = big;
    __syncthreads();
    const bool small = sz != 0 && sz <= KR_BIG_LINE;
    u64 cur = first;
    for (int w = 0; w < KR_BLOCK / 64; w++)
        for (u64 m = s_big[w]; m; m &= m - 1) {
            const int64_t rb = r0 + w * 64 + (__ffsll((long long)m) - 1);
            const u64 b0 = P.rec_out[rb], b1 = P.rec_out[rb + 1];
            kr_range(P, s_tile, cur, b0, small && at >= cur && at < b0, at, sz, g, name_len);
            kr_big_line<REC>(P, s_wave, rb);
            cur = b1;
        }
    kr_range(P, s_tile, cur, last, small && at >= cur, at, sz, g, name_len);
}

// sizes and names of the lines of P.n_reads reads, their exclusive prefix in P.rec_out; totals[0] = bytes, totals[1] = lines (both
// zeroed by the caller)
extern "C" hipError_t gs_launch_kraken_size(const GsKrakenParams *P, hipStream_t stream) {
    const int64_t n_blocks = (P->n_reads + KR_BLOCK - 1) / KR_BLOCK;
    if (n_blocks <= 0) return hipSuccess;
    if (P->rec_line != nullptr)
        hipLaunchKernelGGL(kr_size_kernel<true>, dim3((unsigned)n_blocks), dim3(KR_BLOCK), 0, stream, *P);
    else
        hipLaunchKernelGGL(kr_size_kernel<false>, dim3((unsigned)n_blocks), dim3(KR_BLOCK), 0, stream, *P);
    hipError_t e = gs_launch_scan_blocks(P->rec_block, n_blocks, P->totals, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kr_offsets_kernel, dim3((unsigned)n_blocks), dim3(KR_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

// the text into P.out, which holds totals[0] bytes
extern "C" hipError_t gs_launch_kraken_write(const GsKrakenParams *P, hipStream_t stream) {
    const int64_t n_blocks = (P->n_reads + KR_BLOCK - 1) / KR_BLOCK;
    if (n_blocks <= 0) return hipSuccess;
    if (P->rec_line != nullptr)
        hipLaunchKernelGGL(kr_write_kernel<true>, dim3((unsigned)n_blocks), dim3(KR_BLOCK), 0, stream, *P);
    else
        hipLaunchKernelGGL(kr_write_kernel<false>, dim3((unsigned)n_blocks), dim3(KR_BLOCK), 0, stream, *P);
    return hipGetLastError();
}
