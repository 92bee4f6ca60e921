// gs_rewrite.hip -- the two read-stream goals that neither match nor filter: extract (C/goals/ExtractGoal.java:73-129) and
// fasta2fastq (C/goals/Fasta2FastqGoal.java:92-165).
//
// Selection (extract): one thread per record compares the descriptor line behind its first byte with the key
// (ByteArrayUtil.startsWith, B/util/ByteArrayUtil.java:115-126): selected iff the line holds at least key_len bytes there and
// they equal the key; a '\r' in front of the '\n' belongs to the line.
//
// FASTA -> FASTQ text: per wanted record '@' header[1:] '\n' sequence "\n+\n" '~' x L '\n', back to back in record order; the
// records of general FASTQ chunks the same way, with their own first byte and, where asked for, their quality lines as the tail.
//   ReadEntry mode (AbstractFastqReader.java:375-438, :570-584): the FASTA record search of gs_text.hip has run -- the sequences
//     lie gathered in fa_seq ('\r' kept), off2 holds their bounds, fa_scan / fa_block the prefix over the lines; only the header
//     line of every record is looked up here (rw_emit_kernel), and only records with accept != 0 are written.
//   Goal mode (Fasta2FastqGoal.java:133-164): every trailing '\r' of a data line is stripped with its '\n' (the while at :149-151),
//     empty lines are data lines of zero bytes, every record is written.  The per-line pass is this file's own (the record search
//     refuses empty lines and keeps '\r'): kept length per line by a backward look, the same two-level prefix over the lines, the
//     kept bytes gathered into fa_seq.  A line of 65 534 bytes or more (newline included) is counted, not refused: the reference
//     throws there (AbstractFastaReader.java:104-106), which is the host's to report.
//   Quality mode (goal_mode 2, general FASTQ with qualities, ReadEntry.write with withProbs): the same per-line pass under the
//     line classes of the record search.  A line of class 0 behind a sequence line is the record's '+' line, every further line
//     of class 0 a quality line, kept whole ('\r' included); they are gathered into a buffer of their own (the caller passes it
//     as fa_seq / off2 of this pass and as q_seq / q_off of the copy), so the tail of a record is one run of bytes as its read is.
// General FASTQ records keep the first byte of their descriptor line (keep_first), FASTA records get '@' there.
// Then, for all modes: the size of every record's text, len(header) + L + Q + 5 (Q = L without qualities), an exclusive prefix
// over the records (64-bit: a chunk's output is about twice its input) and the copy.  Records range from 30 bytes to a chromosome, so the copy is cut by
// OUTPUT bytes: a thread owns 16 aligned output bytes, a block 4096; the record of every piece's first byte is found by binary
// search over the offsets (rw_pieces_kernel, all pieces at once), a thread finds its own record between its piece's and the
// next one's.  16 bytes inside one sequence, one '~' run or one quality run -- nearly all of them -- are one 16-byte load and one
// 16-byte store.  Which records are wanted: a per-record byte under a mask and a wanted value, as the four-line gather takes them.
//
//   rw_lines_kernel    goal and quality mode, per line: header? kept length; exclusive scan inside blocks of GS_FA_BLOCK lines
//   rw_scan_kernel     one block: exclusive prefix over per-block totals (lines, then records), optional header count check
//   rw_emit_kernel     per line: header line of every record (both modes); goal mode: off2, destination of the kept bytes
//   rw_gather_kernel   goal and quality mode, one wave per data line: kept bytes -> fa_seq
//   rw_size_kernel     per record: size of its text (0: not wanted), exclusive scan inside blocks of 256 records, records wanted
//   rw_offsets_kernel  per record: + its block's prefix
//   rw_pieces_kernel   per piece of 4096 output bytes: the record of its first byte
//   rw_copy_kernel     the text
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gs_launch.h"
#include "gs_params.h"
#include "gs_scan.h"

#define RW_HDR (1ULL << 40)
#define RW_LEN_MASK (RW_HDR - 1)
#define RW_BLOCK GS_SCAN_BLOCK
#define RW_PIECE (RW_BLOCK * 16)  // output bytes per block and step of the copy
#define RW_LONG_LINE 65534        // bytes incl. the newline from which AbstractFastaReader.readFasta throws (a buffer of 65 535)

// ReadEntry mode reads the FASTA record search's per-block sums (fa_block[blockIdx.x], gs_text.hip) with this file's block index
static_assert(RW_BLOCK == GS_FA_BLOCK, "rw_emit_kernel indexes fa_block by its own blocks: both scans must cut the lines alike");

__device__ __forceinline__ uint32_t rw_line_start(const GsRewriteParams &P, int64_t i) { return i ? P.nl[i - 1] + 1u : 0u; }

// bytes of a data line that the goal prints: the line without its '\n' and without the '\r's in front of it
__device__ __forceinline__ uint32_t rw_kept(const uint8_t *text, uint32_t start, uint32_t len) {
    while (len > 0 && text[(size_t)start + len - 1] == '\r') len--;
    return len;
}

// the per-line pass's view of line i: a header line?  Else the bytes of it that are gathered (goal mode: without trailing '\r's;
// quality mode: a quality line whole, nothing of sequence and '+' lines)
__device__ __forceinline__ bool rw_is_header(const GsRewriteParams &P, int64_t i, uint32_t start, uint32_t len) {
    return P.line_class != nullptr ? P.line_class[i] == 1 : (len > 0 && P.text[start] == '>');
}
__device__ __forceinline__ uint32_t rw_data_len(const GsRewriteParams &P, int64_t i, uint32_t start, uint32_t len) {
    if (P.goal_mode == 2) return i > 0 && P.line_class[i] == 0 && P.line_class[i - 1] == 0 ? len : 0u;
    return rw_kept(P.text, start, len);
}

__global__ __launch_bounds__(RW_BLOCK) void rw_lines_kernel(GsRewriteParams P) {
    __shared__ u64 s_wave[RW_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    const bool live = i < P.n_lines && P.status[GS_TS_CHUNK_ERR] == 0;  // (a count mismatch leaves nl[] partly unwritten)
    u64 v = 0;
    if (live) {
        const uint32_t start = rw_line_start(P, i), len = P.nl[i] - start;
        const bool hdr = rw_is_header(P, i, start, len);
        if (P.goal_mode == 1 && i == 0 && !hdr) {  // text in front of the first header: printed raw by the goal, the host path's case
            atomicOr(&P.status[GS_TS_CHUNK_ERR], GS_TE_SHAPE);
            atomicMin(&P.status[GS_TS_FIRST_BAD], 0u);
        }
        if (P.goal_mode == 1 && len + 1u >= RW_LONG_LINE) atomicAdd(&P.totals[2], 1ULL);
        v = hdr ? RW_HDR : (u64)rw_data_len(P, i, start, len);
    }
    u64 total;
    const u64 ex = gs_block_scan(v, s_wave, &total);
    if (i < P.n_lines) P.fa_scan[i] = ex;
    if (threadIdx.x == 0) P.fa_block[blockIdx.x] = total;
}

// one block: blocks[] -> exclusive prefix in place, *total_out = the sum; expect_hi >= 0: bits 40.. of the sum (the header lines)
// must equal it, else the chunk's counts are wrong
__global__ __launch_bounds__(1024) void rw_scan_kernel(u64 *blocks, int64_t n_blocks, u64 *total_out, int64_t expect_hi, uint32_t *status) {
    __shared__ u64 s_part[1024];
    const int t = threadIdx.x;
    const int64_t per = (n_blocks + 1023) / 1024;
    const int64_t a = std::min<int64_t>((int64_t)t * per, n_blocks), b = std::min<int64_t>(a + per, n_blocks);
    u64 sum = 0;
    for (int64_t i = a; i < b; i++) sum += blocks[i];
    s_part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan
        const u64 x = t >= d ? s_part[t - d] : 0;
        __syncthreads();
        s_part[t] += x;
        __syncthreads();
    }
    u64 run = s_part[t] - sum;
    for (int64_t i = a; i < b; i++) {
        const u64 c = blocks[i];
        blocks[i] = run;
        run += c;
    }
    if (t == 1023) {
        *total_out = s_part[1023];
        if (expect_hi >= 0 && (int64_t)(s_part[1023] >> 40) != expect_hi) atomicOr(&status[GS_TS_CHUNK_ERR], GS_TE_COUNT);
    }
}

__global__ __launch_bounds__(RW_BLOCK) void rw_emit_kernel(GsRewriteParams P) {
    const int64_t i = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    if (i >= P.n_lines || *P.gate != 0) return;
    const uint32_t start = rw_line_start(P, i), len = P.nl[i] - start;
    const bool hdr = rw_is_header(P, i, start, len);
    const u64 pre = P.fa_scan[i] + P.fa_block[blockIdx.x];
    if (i == 0) P.rec_line[P.n_records] = (uint32_t)P.n_lines;
    if (hdr) P.rec_line[pre >> 40] = (uint32_t)i;  // (the header count was checked: pre >> 40 < n_records)
    if (!P.goal_mode) return;
    if (i == 0) P.off2[P.n_records] = P.totals[3] & RW_LEN_MASK;
    if (hdr) {
        P.off2[pre >> 40] = pre & RW_LEN_MASK;
        P.line_dst[i] = 0xffffffffu;
    } else {
        P.line_dst[i] = rw_data_len(P, i, start, len) ? (uint32_t)(pre & RW_LEN_MASK) : 0xffffffffu;
    }
}

__global__ __launch_bounds__(256) void rw_gather_kernel(GsRewriteParams P) {
    if (*P.gate != 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < P.n_lines; i += n_waves) {
        const uint32_t dst = P.line_dst[i];
        if (dst == 0xffffffffu) continue;
        const uint32_t start = rw_line_start(P, i), kept = rw_data_len(P, i, start, P.nl[i] - start);
        for (uint32_t j = (uint32_t)lane; j < kept; j += 64) P.fa_seq[(size_t)dst + j] = P.text[(size_t)start + j];
    }
}

__global__ __launch_bounds__(RW_BLOCK) void rw_size_kernel(GsRewriteParams P) {
    __shared__ u64 s_wave[RW_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    u64 sz = 0;
    if (r < P.n_records && *P.gate == 0 && (P.flags == nullptr || (uint32_t)((P.flags[r] & P.flag_mask) != 0u) == P.flag_want)) {
        const int64_t i = P.rec_line[r];
        const u64 hl = P.nl[i] - rw_line_start(P, i), L = P.off2[r + 1] - P.off2[r];
        sz = hl + L + (P.q_off != nullptr ? P.q_off[r + 1] - P.q_off[r] : L) + 5;
    }
    const u64 wanted = __ballot(sz != 0);
    if ((threadIdx.x & 63) == 0 && wanted) atomicAdd(&P.totals[1], (u64)__popcll(wanted));
    u64 total;
    const u64 ex = gs_block_scan(sz, s_wave, &total);
    if (r < P.n_records) P.rec_out[r] = ex;
    if (threadIdx.x == 0) P.rec_block[blockIdx.x] = total;
}

__global__ __launch_bounds__(RW_BLOCK) void rw_offsets_kernel(GsRewriteParams P) {
    const int64_t r = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    if (r < P.n_records) P.rec_out[r] += P.rec_block[blockIdx.x];
    if (r == 0) P.rec_out[P.n_records] = P.totals[0];
}

// the last record in [lo, hi] whose text starts at or in front of pos (off[lo] <= pos): among records that start at the same byte
// that is the one with text, the others are empty
__device__ __forceinline__ int64_t rw_find(const u64 *off, int64_t lo, int64_t hi, u64 pos) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= pos)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

struct RwRec {
    u64 base, size, hl, L, Q;  // where its text starts, its bytes; header line without '\n', sequence length, bytes of its tail
    size_t hsrc, ssrc, qsrc;   // header line in text, sequence in fa_seq, qualities in q_seq
};
__device__ __forceinline__ RwRec rw_record(const GsRewriteParams &P, int64_t r) {
    RwRec g;
    g.base = P.rec_out[r];
    g.size = P.rec_out[r + 1] - g.base;
    const int64_t i = P.rec_line[r];
    g.hsrc = rw_line_start(P, i);
    g.hl = P.nl[i] - g.hsrc;
    g.ssrc = P.off2[r];
    g.L = P.off2[r + 1] - g.ssrc;
    g.qsrc = P.q_off != nullptr ? P.q_off[r] : 0;
    g.Q = P.q_off != nullptr ? P.q_off[r + 1] - g.qsrc : g.L;
    return g;
}
__device__ __forceinline__ uint8_t rw_byte(const GsRewriteParams &P, const RwRec &g, u64 rel) {
    if (rel < g.hl) return rel == 0 && !P.keep_first ? '@' : P.text[g.hsrc + rel];  // (an empty descriptor line: hl = 0)
    const u64 s = rel - g.hl;  // '\n' sequence '\n' '+' '\n' tail (Q bytes) '\n'
    if (s == 0 || s == g.L + 1 || s == g.L + 3 || s == g.L + g.Q + 4) return '\n';
    if (s <= g.L) return P.fa_seq[g.ssrc + s - 1];
    if (s == g.L + 2) return '+';
    return P.q_seq != nullptr ? P.q_seq[g.qsrc + s - (g.L + 4)] : '~';
}

// the record that holds the first byte of every piece of the text: one search over all records per piece, every piece at once
// (searched by the blocks of the copy, one piece after the other, these ~20 dependent loads were most of its time)
__global__ __launch_bounds__(RW_BLOCK) void rw_pieces_kernel(GsRewriteParams P) {
    const u64 p = (u64)blockIdx.x * RW_BLOCK + threadIdx.x;
    if (p * RW_PIECE < P.totals[0]) P.piece_rec[p] = (uint32_t)rw_find(P.rec_out, 0, P.n_records - 1, p * RW_PIECE);
}

__global__ __launch_bounds__(RW_BLOCK) void rw_copy_kernel(GsRewriteParams P) {
    const u64 total = P.totals[0];
    for (u64 piece = (u64)blockIdx.x * RW_PIECE; piece < total; piece += (u64)gridDim.x * RW_PIECE) {
        const u64 pos = piece + (u64)threadIdx.x * 16;
        if (pos >= total) continue;
        // (the record of the next piece's first byte is not in front of the one of this piece's last byte)
        const int64_t lo = P.piece_rec[piece / RW_PIECE], hi = piece + RW_PIECE < total ? (int64_t)P.piece_rec[piece / RW_PIECE + 1] : P.n_records - 1;
        int64_t r = rw_find(P.rec_out, lo, hi, pos);
        RwRec g = rw_record(P, r);
        u64 rel = pos - g.base;
        uint4 v;
        const u64 seq0 = g.hl + 1, til0 = g.hl + g.L + 4;
        if (rel >= seq0 && rel + 16 <= seq0 + g.L) {
            __builtin_memcpy(&v, P.fa_seq + g.ssrc + (rel - seq0), 16);
        } else if (rel >= til0 && rel + 16 <= til0 + g.Q) {
            if (P.q_seq != nullptr)
                __builtin_memcpy(&v, P.q_seq + g.qsrc + (rel - til0), 16);
            else
                v.x = v.y = v.z = v.w = 0x7e7e7e7eu;
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; j++) {
                if (pos + j < total) {
                    while (rel >= g.size) {  // (behind the last byte of a record there is one with text: pos + j < total)
                        g = rw_record(P, ++r);
                        rel = 0;
                    }
                    w[j >> 2] |= (uint32_t)rw_byte(P, g, rel) << (8 * (j & 3));
                    rel++;
                }
            }
            v.x = w[0];
            v.y = w[1];
            v.z = w[2];
            v.w = w[3];
        }
        *reinterpret_cast<uint4 *>(P.out + pos) = v;  // (the buffer ends on a multiple of 16 behind the text)
    }
}

// extract: accept[r] = the descriptor line of record r behind its first byte starts with the key.  rec_line: the descriptor
// line of every record (FASTA, general FASTQ) or nullptr (four lines per record)
__global__ __launch_bounds__(RW_BLOCK) void rw_select_kernel(const uint8_t *text, const uint32_t *nl, const uint32_t *rec_line, int64_t n_records,
                                                            const uint8_t *key, int32_t key_len, const uint32_t *skip, uint8_t *accept) {
    const int64_t r = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    if (r >= n_records || *skip != 0) return;  // (a refused chunk: the flags stay zero)
    const int64_t i = rec_line ? (int64_t)rec_line[r] : 4 * r;
    const uint32_t start = i ? nl[i - 1] + 1u : 0u, len = nl[i] - start;
    bool hit = (int64_t)len - 1 >= (int64_t)key_len;
    for (int32_t j = 0; hit && j < key_len; j++) hit = text[(size_t)start + 1 + j] == key[j];
    accept[r] = hit ? 1 : 0;
}

// goal mode, in front of the commit of the chunk (P.gate = the bank's chunk error word): lines, header count, header lines and
// sequence bounds, kept bytes -> fa_seq.  The newline offsets are there (gs_launch_text_lines); totals[2] has been zeroed.
// Quality mode, behind the commit of a general FASTQ chunk (P.gate = the bank's skip flag, n_lines = the lines its whole records
// cover, n_records = their number, which the record search has made the number of class-1 lines): the same for the quality lines.
extern "C" hipError_t gs_launch_rewrite_lines(const GsRewriteParams *P, hipStream_t stream) {
    const int64_t n_blocks = (P->n_lines + RW_BLOCK - 1) / RW_BLOCK;
    if (n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(rw_lines_kernel, dim3((unsigned)n_blocks), dim3(RW_BLOCK), 0, stream, *P);
    hipLaunchKernelGGL(rw_scan_kernel, dim3(1), dim3(1024), 0, stream, P->fa_block, n_blocks, P->totals + 3, P->goal_mode == 1 ? P->n_records : (int64_t)-1,
                       P->status);
    hipLaunchKernelGGL(rw_emit_kernel, dim3((unsigned)n_blocks), dim3(RW_BLOCK), 0, stream, *P);
    hipLaunchKernelGGL(rw_gather_kernel, dim3((unsigned)std::min<int64_t>((P->n_lines + 3) / 4, 8192)), dim3(256), 0, stream, *P);
    return hipGetLastError();
}

// the header line of every record of a chunk the record search has accepted (P.gate = the bank's skip flag)
extern "C" hipError_t gs_launch_rewrite_heads(const GsRewriteParams *P, hipStream_t stream) {
    const int64_t n_blocks = (P->n_lines + RW_BLOCK - 1) / RW_BLOCK;
    if (n_blocks > 0) hipLaunchKernelGGL(rw_emit_kernel, dim3((unsigned)n_blocks), dim3(RW_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

// sizes, offsets and the text of the wanted records into P.out (room for out_bound bytes, a multiple of 16); totals[0] = bytes,
// totals[1] = records (both zeroed by the caller).  P.gate = the bank's skip flag: a refused chunk gives no text.
extern "C" hipError_t gs_launch_rewrite_copy(const GsRewriteParams *P, int64_t out_bound, int n_cu, hipStream_t stream) {
    const int64_t n_blocks = (P->n_records + RW_BLOCK - 1) / RW_BLOCK;
    if (n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(rw_size_kernel, dim3((unsigned)n_blocks), dim3(RW_BLOCK), 0, stream, *P);
    hipLaunchKernelGGL(rw_scan_kernel, dim3(1), dim3(1024), 0, stream, P->rec_block, n_blocks, P->totals, (int64_t)-1, (uint32_t *)nullptr);
    hipLaunchKernelGGL(rw_offsets_kernel, dim3((unsigned)n_blocks), dim3(RW_BLOCK), 0, stream, *P);
    const int64_t pieces = (out_bound + RW_PIECE - 1) / RW_PIECE;
    hipLaunchKernelGGL(rw_pieces_kernel, dim3((unsigned)((pieces + RW_BLOCK - 1) / RW_BLOCK)), dim3(RW_BLOCK), 0, stream, *P);
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(pieces, (int64_t)n_cu * 8));
    hipLaunchKernelGGL(rw_copy_kernel, dim3(grid), dim3(RW_BLOCK), 0, stream, *P);
    return hipGetLastError();
}

// blocks[0 .. n_blocks) -> their exclusive prefix in place, *total_out = the sum (one block of 1024 threads)
extern "C" hipError_t gs_launch_scan_blocks(u64 *blocks, int64_t n_blocks, u64 *total_out, hipStream_t stream) {
    hipLaunchKernelGGL(rw_scan_kernel, dim3(1), dim3(1024), 0, stream, blocks, n_blocks, total_out, (int64_t)-1, (uint32_t *)nullptr);
    return hipGetLastError();
}

extern "C" hipError_t gs_launch_select(const uint8_t *text, const uint32_t *nl, const uint32_t *rec_line, int64_t n_records, const uint8_t *key,
                                       int32_t key_len, const uint32_t *skip, uint8_t *accept, hipStream_t stream) {
    const int64_t n_blocks = (n_records + RW_BLOCK - 1) / RW_BLOCK;
    if (n_blocks > 0)
        hipLaunchKernelGGL(rw_select_kernel, dim3((unsigned)n_blocks), dim3(RW_BLOCK), 0, stream, text, nl, rec_line, n_records, key, key_len, skip, accept);
    return hipGetLastError();
}
