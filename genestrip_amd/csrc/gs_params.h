// gs_params.h -- kernel parameter blocks and launch constants shared by the kernel units and gs_api.cpp
#pragma once
#include <stdint.h>

#include "../../include/gsgpu.h"
#include "gs_layout.h"
#include "gs_snrec.h"

#define GS_BLOCK 256   // 4 waves per workgroup
#ifndef GS_NV_LDS
#define GS_NV_LDS 128  // per-taxid counters are privatised in LDS up to this many value indices: 25 values 10.2 ms in LDS against 49 ms with global atomics on 25 hot counters; 211 values 11.5 ms in LDS (the footprint costs occupancy) against 10.7 ms global
#endif
#define GS_NV_TREE_LDS 2048   // up to here the taxonomy arrays (12 B per value) still travel in LDS
#define GS_STAT_REC_MAX_VALUES 10240  // deferred statistics (GsStatRec): at most 16 passes of 640 values over the records

// Deferred statistics of a read whose hit k-mers all carry ONE tax id (the usual case).  When the per-taxid counters do
// not fit the LDS, such a read writes this record instead of ~20 global atomics, and gs_stat_reduce_kernel adds the
// records up in LDS tables of its own (a kernel that has the whole LDS for them).
struct GsStatRec {
    int32_t vi;          // value index, -1: nothing deferred (no hit, several tax ids, long read)
    int32_t contigs;
    int64_t kmers;
    int64_t sq;          // sum of squared contig lengths
    uint64_t max_key;    // (longest contig << 40) | (2^40 - 1 - read number)
    int32_t counted;     // 1: the read was classified to vi and passed the class-error gate
    int32_t read_kmers;
    int32_t read_len;
    int32_t n_pos;       // k-mer positions of the read (`max` of matchRead)
    // the error quotients tax_err / n_pos and (n_pos - read_kmers) / n_pos are formed by gs_stat_reduce_kernel, one thread per
    // record: in the match kernel a division on lane 0 costs what 64 cost
    int32_t tax_err;
    int32_t pad[3];      // (64 bytes: a record never straddles two cache lines)
};
static_assert(sizeof(GsStatRec) == 64, "GsStatRec");

// (GsQuotTable -- gates and quotients of a batch of one read length -- and GsSnRec: gs_snrec.h)

struct GsMatchParams {
    GsDbDev db;
    const uint8_t *seq;
    const uint64_t *off;
    int64_t n_reads;
    int64_t first_read_no;
    int32_t classify, count_unique, max_paths, threshold;
    double max_read_tax_err, max_read_class_err;
    int64_t *sums;         // [n_values][GS_N_SUMS]
    int64_t *max_keys;     // [n_values]
    double *dsums;         // [n_values][GS_N_DCOLS]
    uint32_t *bitmap;      // one bit per table slot
    uint32_t *hit_counts;  // per table slot, or nullptr (maxKMerResCounts == 0)
    int32_t *class_vi;     // optional per read
    uint8_t *flags;        // optional per read
    unsigned int *long_count;  // [0] entries of the queue of reads with more than 128 k-mer positions (chunks of 64 per wave), [1] the long-read kernel's chunk cursor
    uint32_t *long_list;
    // DB-partitioned mode only: node of every k-mer position, looked up by the owning rank (nullptr: probe locally)
    const int32_t *nodes;
    const unsigned long long *pos_off;  // n_reads + 1: first position of read r in `nodes`
    // text mode (gs_match_submit_text): `off` holds (start, end) PAIRS of the in-place sequence lines (off_stride 2,
    // else 1: n_reads + 1 running offsets), and the whole launch is skipped when *skip != 0 (chunk refused by the
    // device-side record scan, gs_text.hip)
    // off_stride 0: NO offsets at all -- every read is fixed_len bytes, read r at r * fixed_len (gs_match_submit_fixed): the offsets'
    // round trip in front of the bases' (14 % of a wave's cycles on a store that does not fit the caches) is gone
    int32_t off_stride;
    int32_t fixed_len;
    // != 0: the waves take the FIXED loop WITHOUT the minimizer gate (gs_probe_planes<.., NOGATE>): set by launch_batch for batches
    // behind the prefilter; gs_launch_match refuses it where that loop cannot be taken
    int32_t fixed_nogate;
    // direct global-atomic counters (n_values > GS_NV_LDS) exist in `stat_copies` copies, one per group of workgroups
    // (blockIdx % stat_copies): the atomics of one tax id are spread over that many cache lines; the copies are
    // folded into copy 0 before anything reads the accumulators
    int32_t stat_copies;
    const uint32_t *skip;
    // gates and quotients of this batch's one read length (the FIXED loop of gs_match_kernel reads nothing else of them), or nullptr:
    // a batch with offsets, a length that loop does not take
    const GsQuotTable *quot;
    GsStatRec *stat_recs;  // deferred statistics (global-atomic counters only) or nullptr: room for n_reads + 64 per wave
    unsigned long long *stat_rec_count;  // records handed out so far (waves take them 64 at a time)
    // Reads of huge_min k-mer positions and more (assembled contigs, chromosomes: the reference grows its read buffer for them,
    // AbstractFastqReader.java:593-604) are taken apart over MANY waves: the long-read kernel hands the first huge_slots of a batch
    // to gs_match_huge_kernel (chunks of whole iterations, one wave each; per read: vote counts and first positions per node, the
    // runs at the chunks' ends) and gs_match_huge_finish_kernel puts each read together again (seams, distinct nodes in order of first
    // appearance, classification).  nullptr: off (DB-partitioned mode, batches of short fixed-length reads).
    unsigned int *huge_count;          // reads handed over so far
    uint32_t *huge_list;               // [huge_slots] their numbers in the batch
    struct GsHugeHead *huge_head;      // [huge_slots][GS_HUGE_COPIES]
    struct GsHugeChunk *huge_chunks;   // [huge_slots][GS_HUGE_MAX_CHUNKS]
    uint32_t *huge_cnt;                // [huge_slots][GS_HUGE_COPIES][n_values] positions that hold the node (chunk c votes on copy c mod GS_HUGE_COPIES)
    uint32_t *huge_first;              // [huge_slots][GS_HUGE_COPIES][n_values] its first position (~0: none)
    uint32_t *huge_touch;              // [huge_slots][GS_HUGE_COPIES * n_values] the nodes with a count, in no order, once per copy (GsHugeHead.n_touch of them)
    uint32_t *huge_fold;               // [huge_slots][2][n_values] the copies folded by the finish kernel: votes, first position
    // long_count: three queues x (entries, cursor) -- queue 0 the long-read kernel's, queues 1 / 2 those of gs_match_wide_kernel<3 / 4>
    // (reads of 129 .. 192 / 193 .. 256 positions, where wide_mask says that kernel serves this run); long_list: queue q at q * long_cap
    int64_t long_cap;
    int32_t wide_mask;
    int32_t pad2;
    int32_t huge_slots;                // <= GS_HUGE_SLOTS
    int32_t huge_min;                  // k-mer positions from which a read goes this way
    int32_t huge_chunk_min;            // k-mer positions per chunk at least (a multiple of 128)
    int32_t pad1;
    // The FIXED loop of gs_match_kernel behind the prefilter (gs_prefilter.hip): trip i of the launch takes read surv_list[i], and
    // there are *surv_count of them (both written by gs_pf_kernel on the same stream).  nullptr: every read of the batch, in order.
    const uint32_t *surv_list;
    const uint32_t *surv_count;
    // The FIXED loop with counters in LDS only looks k-mers up: every read writes sn_recs[t] (t: the trip, i.e. the index into
    // surv_list, or the read's number) and books nothing; a read of several tax ids or with a non-CGAT byte also writes row t of
    // sn_nodes (GS_SN_ROW 16-bit node codes, gs_snrec.h).  gs_sn_reduce_kernel and gs_sn_walk_kernel follow on the same stream.
    // Either pointer nullptr: a batch of one length takes the general loop, where the wave that probed a read books it.
    GsSnRec *sn_recs;
    uint16_t *sn_nodes;
};

// gs_snreduce.hip: the records of a batch into the run's counters and per-read outputs, one lane per record
struct GsSnReduceParams {
    const GsSnRec *recs;
    const uint32_t *count;     // records of the launch: *count (the survivors of the prefilter), nullptr: n_reads
    int64_t n_reads;
    int64_t first_read_no;
    GsSnConst c;
    int32_t n_values, stat_copies;
    const GsQuotTable *quot;
    int64_t *sums;             // the run's counters in stat_copies copies, as GsMatchParams
    int64_t *max_keys;
    double *dsums;
    int32_t *class_vi;         // per-read outputs of the batch or nullptr
    uint8_t *flags;
    unsigned int *booked;      // += records with vi >= 0 (one atomic per workgroup)
    // the slots of the records with vi == GS_SN_NODES, densely, for gs_sn_walk_kernel (room for n_reads), and their number
    uint32_t *row_list;
    unsigned int *n_rows;      // += (one atomic per workgroup)
    // gs_sn_walk_kernel alone: the rows of node codes and what the walk needs of the run's settings
    const uint16_t *nodes;
    const int32_t *parent, *tin, *tout;
    int32_t max_paths, pad;
};
// words behind the run's counters: three queues x (entries, cursor), the prefilter's survivors, the records booked, the rows listed
#define GS_QUEUE_WORDS 10
#define GS_HUGE_MIN (1 << 15)
#define GS_HUGE_SLOTS 256       // (= GS_BLOCK: one thread per slot where the chunks are counted)
#define GS_HUGE_MAX_CHUNKS 8192
#define GS_HUGE_COPIES 16      // of a read's vote rows and counters (a power of two, at most 64)
#define GS_HUGE_CHUNK_MIN 1024  // a longer read than GS_HUGE_MAX_CHUNKS of these is cut into GS_HUGE_MAX_CHUNKS chunks
struct GsHugeHead {
    unsigned int n_miss, bad_lo, flags, n_touch;  // flags: 1 = some k-mer hit, 2 = a bad base at or behind position max - 1
};
struct GsHugeChunk {
    int32_t head_node, head_len;  // the run the chunk starts with (it may continue the chunk before): node, positions
    int32_t tail_node, tail_len;  // the run that is open at its end; tail_len < 0: the whole chunk is ONE run (head_len positions)
};

// device-side FASTQ record scan (gs_text.hip)
enum { GS_TS_STICKY = 0, GS_TS_CHUNK_ERR = 1, GS_TS_FIRST_BAD = 2, GS_TS_SKIP = 3, GS_TS_FAILED_TICKET = 4, GS_TS_WORDS = 8 };
enum { GS_TE_NUL = 1, GS_TE_COUNT = 2, GS_TE_SHAPE = 4 };

struct GsTextParams {
    const uint8_t *text;   // n_bytes, padded with blanks to a multiple of 4096
    int64_t n_bytes;
    int64_t n_lines;       // newlines the host counted (a multiple of 4)
    uint32_t *tile_count;  // one per 4096-byte tile
    uint32_t *nl;          // n_lines newline offsets
    unsigned long long *off2;          // 2 * (n_lines / 4): (start, end) of every record's sequence line
    unsigned long long *chunk_totals;  // [3] scratch: -, k-mers, bases of this chunk
    unsigned long long *run_totals;    // [3] reads, k-mers, bases accepted so far
    uint32_t *status;      // GS_TS_WORDS words
    int32_t k;
    int32_t pad;
    // FASTA mode (gs_match_submit_fasta): n_records > = 0 header lines expected, reads gathered into fa_seq
    int64_t n_records;                // -1: FASTQ mode
    unsigned long long *fa_scan;      // per line: exclusive prefix inside its block of (header ? 1 << 40 : length)
    unsigned long long *fa_block;     // per block of GS_FA_BLOCK lines: total, then exclusive prefix
    uint32_t *line_dst;               // per line: destination of its bytes in fa_seq, ~0 for header lines
    uint8_t *fa_seq;                  // the sequences of the chunk's records back to back; off2[0 .. n_records] = their bounds
    // general FASTQ (gs_match_submit_fastq_ml: sequence and quality over any number of lines): the record structure is found
    // on the device first, then the FASTA kernels gather the sequence lines under these classes
    const uint8_t *line_class;        // per line: 1 descriptor line, 2 sequence line, 0 anything else; nullptr in the other modes
    uint32_t *ml_next, *ml_plus;      // per line i, IF a record starts there: the line behind its last quality line, its '+' line
    uint32_t *ml_jump_a, *ml_jump_b;  // pointer doubling
    uint8_t *ml_mark;                 // 1: a record starts at this line
    unsigned long long *ml_out;       // [0] complete records [1] lines they cover [2] bytes they cover
};
#define GS_ML_NONE 0xffffffffu
#define GS_ML_TOO_LONG 0xfffffffeu
#define GS_ML_MAX_LINES 4096  // lines one record may span before the chunk is refused (the host parser takes over)
#define GS_FA_BLOCK 256

// extract and fasta2fastq (gs_rewrite.hip): the text of FASTA records as four-line FASTQ, behind the record search of gs_text.hip
// (ReadEntry mode) or behind the newline scan alone (goal mode, goal_mode != 0)
struct GsRewriteParams {
    const uint8_t *text;              // the chunk, as GsTextParams
    int64_t n_lines, n_records;
    const uint32_t *nl;
    const uint8_t *line_class;        // general FASTQ (header lines for the selection only) or nullptr
    unsigned long long *fa_scan, *fa_block;  // as GsTextParams: read in ReadEntry mode, written in goal mode
    uint32_t *line_dst;               // goal mode: destination of a data line's kept bytes in fa_seq, ~0: none
    uint8_t *fa_seq;                  // the sequences back to back; off2[0 .. n_records] = their bounds
    unsigned long long *off2;
    uint32_t *status;                 // the bank's GS_TS_WORDS words
    const uint32_t *gate;             // the launch does nothing when *gate != 0: the chunk error word in front of the commit, the skip flag behind it
    int32_t goal_mode;                // 0: ReadEntry mode; 1: fasta2fastq; 2: the quality lines of a general FASTQ chunk (line_class set) -> fa_seq / off2
    int32_t keep_first;               // the descriptor line keeps its first byte (general FASTQ); 0: it becomes '@' (FASTA)
    const uint8_t *flags;             // per record, nullptr: every record; else a record is wanted iff ((flags[r] & flag_mask) != 0) == flag_want
    uint32_t flag_mask, flag_want;
    const uint8_t *q_seq;             // the quality characters of every record back to back, q_off[0 .. n_records] = their bounds
    const unsigned long long *q_off;  // (the gather of a goal_mode 2 pass); nullptr: the tail is '~' x L
    uint32_t *rec_line;               // n_records + 1: the header line of every record, then n_lines
    unsigned long long *rec_out;      // n_records + 1: where the text of every record starts
    unsigned long long *rec_block;    // per block of 256 records
    uint32_t *piece_rec;              // per 4096 bytes of the text: the record that holds the first of them
    unsigned long long *totals;       // [0] bytes of text [1] records written [2] lines of 65 534 bytes and more [3] scratch
    uint8_t *out;
};

// Kraken-style lines of a chunk as device text (gs_kraken.hip), behind the segments of the chunk's reads
struct GsKrakenParams {
    const uint8_t *text;              // the chunk and its newline offsets, as GsTextParams
    const uint32_t *nl;
    int64_t n_reads;
    int32_t k, write_all;
    const int32_t *cls;               // per read: value index of its class, < 0: unclassified
    const unsigned long long *seg_off;  // n_reads + 1; the segments of read r: [seg_off[r], seg_off[r + 1])
    const int32_t *seg_code;          // value index, -1: no hit, -2: a window with a bad base
    const int32_t *seg_start;
    const uint8_t *tax_bytes;         // taxid of value v: tax_bytes[tax_off[v] .. tax_off[v + 1])
    const uint32_t *tax_off;
    uint32_t *name_len;               // per read: bytes of its name (descriptor behind its first byte, up to the first blank)
    unsigned long long *rec_out;      // n_reads + 1: where the line of every read starts (a read without a line: an empty one)
    unsigned long long *rec_block;    // per block of 256 reads
    unsigned long long *totals;       // [0] bytes of text [1] lines
    uint8_t *out;
    // (behind the fields of the four-line form, whose kernel arguments keep their places)
    const uint32_t *rec_line;         // FASTA, general FASTQ: the descriptor line of every read; nullptr: four lines per read
    const unsigned long long *off2;   // with rec_line: n_reads + 1 bounds of the gathered reads (their lengths)
};

struct GsFilterParams {
    int32_t kind;           // GS_BLOOM_*
    int32_t k;
    int32_t min_pos_count;
    int32_t n_hashes;
    double positive_ratio;
    uint64_t bits;          // XOR/Murmur: bit count ; Blocked: bucket count
    uint64_t magic;         // unsigned division of a 64-bit value by `bits` (round-up method)
    int32_t magic_shift;    // ceil(log2(bits))
    int32_t pad;
    const unsigned long long *words;
    const int64_t *factors;
    const uint8_t *seq;
    const uint64_t *off;
    int64_t n_reads;
    uint8_t *accept;
    int32_t off_stride;     // 1: running offsets; 2: (start, end) pairs (text mode, gs_text.hip)
    int32_t pad2;
    const uint32_t *skip;   // text mode: the launch does nothing when *skip != 0
};

// gs_index.hip: the index filter built from a handle's store (BloomIndexGoal).  The store part is what GsExportParams holds.
struct GsIndexParams {
    const unsigned long long *rec;  // this handle's record lines, n_rec of them
    int64_t n_rec;
    const unsigned long long *tab;  // this handle's table buckets: global buckets tab_first ..
    int64_t tab_first, n_tab;
    uint32_t bucket_bits, vbits;
    int32_t k, n_values;
    const uint32_t *requested;      // one bit per value index: bit (v & 31) of word v >> 5
    int32_t put;                    // 0: count the selected k-mers only
    int32_t kind;                   // GS_BLOOM_*
    int32_t n_hashes;
    uint32_t hash_inv;              // ceil(2^32 / n_hashes) for n_hashes >= 2: pair p -> key p / n_hashes without a division
    uint64_t bits;                  // XOR/Murmur: bit count ; Blocked: bucket count
    uint64_t magic;                 // gs_absmod.h: unsigned division by `bits`
    int32_t magic_shift;
    int32_t pad;
    const int64_t *factors;         // n_hashes hash factors; Blocked: factors[0] = the seed
    unsigned long long *words;
    unsigned long long *count;      // selected k-mers (one atomic per wave)
};

// gs_prefilter.hip: the 15-mer filter of a store (gs_prefilter.h) ...
struct GsPrefilterBuildParams {
    const unsigned long long *rec;  // the store's record lines, n_rec of them
    int64_t n_rec;
    const unsigned long long *tab;  // its table buckets, n_tab of them
    int64_t n_tab;
    uint32_t bucket_bits, vbits;
    int32_t k, pad;
    uint32_t *l1, *l2;              // both levels, zeroed by the caller
    unsigned long long *count;      // |S|: the set bits of the exact level (zeroed by the caller)
};
// ... and the test of a batch of one read length against it
struct GsPrefilterParams {
    const uint8_t *seq;             // n_reads reads of L bytes, back to back
    int64_t n_reads;
    int32_t L, k;
    const uint32_t *l1, *l2;
    uint32_t *list;                 // the reads that pass, in no order (room for n_reads)
    uint32_t *count;                // how many (zeroed by the caller)
    int32_t *class_vi;              // per-read outputs of the batch or nullptr: a rejected read gets -1 / 0 here
    uint8_t *flags;
};

struct GsSegParams {
    GsDbDev db;
    const uint8_t *seq;
    const uint64_t *off;
    int64_t n_reads;
    uint32_t *seg_count;            // count pass: segments per read
    const unsigned long long *seg_off;  // write pass: exclusive prefix of seg_count
    int32_t *seg_code;
    int32_t *seg_start;
    int32_t off_stride;  // 1: running offsets; 2: (start, end) pairs (text mode)
    int32_t huge_min;    // reads of this many k-mer positions and more are left out (count pass: seg_count = GS_SEG_HUGE) ...
    // ... and come back cut into pieces of whole iterations, one wave each (a chromosome on one wave: 150 ms per 5 Mbp and pass)
    const struct GsSegPiece *pieces;
    struct GsSegPieceOut *piece_out;  // count pass
    int64_t n_pieces;
};
#define GS_SEG_HUGE 0xffffffffu
#define GS_SEG_PIECE_ITERS 32  // iterations (of 128 positions) per piece
struct GsSegPiece {
    uint32_t read;
    int32_t it0, n_iter;  // its iterations
    int32_t carry;        // write pass: the node of the position in front of it (GS_NODE_NONE: the read starts here)
    unsigned long long out_off;  // write pass: where its first run goes, relative to the read's first
};
struct GsSegPieceOut {
    int32_t first_node, last_node;  // of its first and its last position
    uint32_t count, pad;            // runs that start in it, its first position taken as a start
};

struct GsEncodeParams {
    int32_t k;
    int32_t pad;
    const uint8_t *seq;
    const uint64_t *off;
    int64_t n_reads;
    const unsigned long long *pos_off;  // n_reads + 1 (exclusive prefix of max(0, L-k+1))
    unsigned long long *keys;           // gs_mix62(canonical planar key), ~0 for windows with a non-CGAT base,
                                        // ~0 - 1 for k-mers the minimizer gate rules out
    const uint32_t *mgate;              // the store's minimizer gate (covers every partition's keys) or NULL
    uint32_t mgate_bits;
    uint32_t pad2;
};

// fused encode + routing of the DB-partitioned mode (gs_encode_route_kernel): owner o's keys go to
// send_keys[o * cap ..), handed out to the waves in chunks of GS_ROUTE_CHUNK slots; idx = position of the key in the
// batch (~0: a slot that was handed out but not used, its key is the invalid-window sentinel)
#define GS_ROUTE_CHUNK 2048
struct GsRouteParams {
    int32_t n_parts;
    int32_t pad;
    unsigned long long cap;        // slots per owner region (a multiple of GS_ROUTE_CHUNK)
    unsigned long long *cursors;   // [n_parts] slots handed out per owner; [64] = overflow flag
    unsigned long long *send_keys;
    uint32_t *send_idx;
    int32_t *nodes;                // per k-mer position: node of the positions that are not routed
};

// ---- gs_krakencount.hip: Kraken-style lines counted per tax id (the krakencount goal)
#define GS_KC_TILE 4096        // bytes per scan block: GS_SCAN_BLOCK threads, 16 bytes each
#define GS_KC_GROUP 8          // scan blocks per workgroup of the accumulation: its LDS table is flushed once per GS_KC_TILE * GS_KC_GROUP bytes
#define GS_KC_LDS_SLOTS 512    // slots of that table (28 bytes each)
#define GS_KC_LDS_PROBES 32    // a key that finds no slot within this many steps goes straight to the global table
#define GS_KC_EMPTY 0xffffffffu  // no key (accepted tax ids have at most 9 digits), no line
#define GS_KC_LONG_LINE 65536  // bytes incl. the newline beyond which KrakenResultProcessor (a line buffer of 65 536) fails
enum { GS_KC_READS = 0, GS_KC_KMERS = 1, GS_KC_KIMR = 2 };  // the three counters of a row, in the order of the CSV
// chunk status words: reset by the finish kernel for the next chunk
enum { GS_KC_BAD_LINE = 0,    // first line outside the grammar (GS_KC_EMPTY: none)
       GS_KC_EMPTY_LINE = 1,  // first empty line ...
       GS_KC_EMPTY_OFF = 2,   // ... and its byte offset
       GS_KC_FULL = 3,        // the table cannot take the chunk's new tax ids
       GS_KC_WORDS = 4 };
// what the finish kernel reports per chunk
enum { GS_KC_R_REFUSED = 0,   // 0: counted; 1: outside the grammar; 2: table full
       GS_KC_R_BAD_LINE = 1, GS_KC_R_EMPTY_OFF = 2, GS_KC_R_ROWS = 3,  // (~0: none); rows of the table
       GS_KC_R_CHUNK = 4,     // [4] lines, counted tokens, 'A' tokens, long lines of this chunk (zeros if refused)
       GS_KC_R_RUN = 8,       // [4] the same since the last reset
       GS_KC_R_WORDS = 12 };
struct GsKrakenCountParams {
    const uint8_t *text;      // n_bytes of whole lines, zero bytes behind them up to n_tiles * GS_KC_TILE + 64
    int64_t n_bytes, n_tiles;
    unsigned long long *tile_lt;  // per scan block: newlines | tabs << 32, then their exclusive prefix (gs_launch_scan_blocks)
    unsigned long long *tile_c;   // the same for token candidates (a digit behind a blank or a tab)
    unsigned long long *scan_tot; // [2] the sums
    uint32_t *line_end;       // per line (line_cap of them): offset of its newline ...
    uint32_t *line_c4;        // ... candidates in front of its fourth tab ...
    uint32_t *line_key;       // ... and its class tax id
    int64_t line_cap;
    uint32_t *status;         // GS_KC_WORDS
    unsigned long long *chunk_tot, *run_tot;  // lines, counted tokens, 'A' tokens, long lines (chunk_tot: and the two of `counters`)
    uint32_t *keys;           // the table: n_slots keys (GS_KC_EMPTY: free), open addressing, linear probing
    uint32_t *present;        // 1: the row exists; 0 with a key: claimed by the chunk under way
    unsigned long long *acc, *delta;  // 3 counters per slot: the committed rows, what the chunk under way adds
    uint32_t n_slots, slot_bits, max_keys, pad;
    uint32_t *n_keys;         // [0] rows committed [1] rows committed + claimed
    unsigned long long *counters;  // [0] global atomics of the accumulation [1] tokens whose key went straight to the global table
    unsigned long long *result;    // GS_KC_R_WORDS
};

// ---- gs_genomes.hip: genome FASTA text -> regions of the kept records
#define GS_GN_TILE 4096   // bytes per tile: GS_SCAN_BLOCK threads, 16 bytes each; the piece of the gather
#define GS_GN_CR_CAP 64   // a run of more '\r' than this refuses the chunk (the look-ahead behind a '\r' is bounded by it)
#define GS_GN_MAX_RECORDS (1 << 24)  // header lines of a chunk stay below this: the selection scan packs kept records << 40 | bases
#define GS_GN_PAD 128     // '\n' bytes behind the last tile of the text: the look-ahead reads up to GS_GN_CR_CAP + 1 bytes on
enum { GS_GN_NUL = 0,      // status: offset of the first NUL byte (~0: none)
       GS_GN_CR = 1,       // offset of the first run of more than GS_GN_CR_CAP '\r' (~0: none)
       GS_GN_MAXLINE = 2,  // the longest line in front of the cut, its newline included
       GS_GN_WORDS = 4 };
enum { GS_GN_R_CUT = 0,        // res: bytes the records that end inside the chunk cover
       GS_GN_R_HDR_BYTES = 1,  // bytes of their header lines
       GS_GN_R_KEPT = 2,       // kept records << 40 | their bases
       GS_GN_R_WORDS = 4 };
struct GsGenomesParams {
    const uint8_t *text;          // n_bytes, then '\n' up to n_tiles * GS_GN_TILE + GS_GN_PAD
    int64_t n_bytes, n_tiles;
    int32_t last, pad;            // last != 0: the stream ends with this chunk
    unsigned long long *tile_hl;  // n_tiles + 1: header lines << 32 | newlines per tile, then their exclusive prefix and the sum
    unsigned long long *tile_c;   // the same for content bytes
    uint32_t *status;             // GS_GN_WORDS
    unsigned long long *res;      // GS_GN_R_WORDS
    int64_t n_hdr, n_nl;          // header lines and newlines of the chunk (the sums, read back by the caller)
    int64_t n_records;            // records that end inside the chunk: n_hdr, without `last` one less
    uint32_t *nl, *cnl;           // per newline: its offset, the content bytes in front of it
    uint32_t *rec_start, *rec_line;   // per header line: its offset, its line number
    uint32_t *base_start, *base_cnt;  // per record: content index of its first base, its bases
    unsigned long long *hdr_off;      // n_records + 1: where its header line goes in hdr_out
    unsigned long long *rec_block;    // per block of GS_SCAN_BLOCK records: the sums of the scans over the records
    uint8_t *hdr_out;
    const uint8_t *keep;          // n_records flags, or nullptr: every record
    unsigned long long *sel;      // n_records + 1: kept records << 40 | their bases in front of each record
    unsigned long long *off;      // kept + 1: the regions' offsets
    uint8_t *seq;                 // their bases
};

// ---- gs_accmap.hip: RefSeq catalog lines -> accession map (the accmapsize / accmap goals)
#define GS_AM_TILE 4096       // bytes per scan block: GS_SCAN_BLOCK threads, 16 bytes each
#define GS_AM_MAX_LINE 2048   // bytes of a line with its newline beyond which AccessionFileProcessor throws
#define GS_AM_MAX_KEY 31      // accession bytes a 32-byte slot holds behind its length byte
#define GS_AM_MAX_PATTERNS 16 // category strings, and status strings
#define GS_AM_MAX_PATTERN 32  // bytes of one of them
#define GS_AM_NONE 0xffffffffu
enum { GS_AM_BAD_LINE = 0,    // status: first line outside the grammar (GS_AM_NONE: none)
       GS_AM_LONGEST = 1,     // the longest line, its newline included
       GS_AM_WORDS = 2 };
enum { GS_AM_C_LINES = 0, GS_AM_C_PASSING = 1, GS_AM_C_PUT = 2, GS_AM_C_WORDS = 4 };  // the chunk's counters
struct GsAccmapPatterns {     // [0 .. n_cat): categories, [GS_AM_MAX_PATTERNS .. GS_AM_MAX_PATTERNS + n_stat): statuses
    uint8_t len[2 * GS_AM_MAX_PATTERNS];
    uint8_t text[2 * GS_AM_MAX_PATTERNS][GS_AM_MAX_PATTERN];
};
struct GsAccmapParams {
    const uint8_t *text;          // n_bytes of whole lines, zero bytes behind them up to n_tiles * GS_AM_TILE + 64
    int64_t n_bytes, n_tiles;
    int32_t last;                 // != 0: the stream ends with this chunk, whose final line need not be terminated
    int32_t dna, rna, mrna;       // the accession prefixes that pass
    int32_t n_cat, n_stat;
    const GsAccmapPatterns *pat;
    const int32_t *known;         // n_nodes tax ids, ascending
    int32_t n_nodes, pad;
    unsigned long long *tile_lt;  // per tile: newlines | tabs << 32, then their exclusive prefix (gs_launch_scan_blocks)
    uint32_t *tile_tail;          // per tile: (offset of its last newline + 1, 0: none) | tabs behind that newline << 16
    unsigned long long *tile_put; // per tile: entries it puts, then their exclusive prefix
    unsigned long long *scan_tot; // [2] the sums
    uint32_t *status;             // GS_AM_WORDS
    unsigned long long *chunk;    // GS_AM_C_WORDS
    uint8_t *keys;                // the write pass: 32-byte slots, entry_cap of them ...
    int32_t *nodes;               // ... their nodes
    int64_t first_entry, entry_cap;  // the chunk's first entry goes to slot first_entry
    int32_t *regions;             // n_nodes: entries per node
};

// ---- gs_asmsum.hip: Genbank assembly summary lines -> per-node picks (the fastasgenbank goal)
#define GS_AS_TILE 4096       // bytes per scan block: GS_SCAN_BLOCK threads, 16 bytes each
#define GS_AS_MAX_LINE 4096   // bytes of a line with its newline beyond which the device refuses the chunk
#define GS_AS_NONE 0xffffffffu
#define GS_AS_LINE_BLOCK 256  // lines per judging block (GS_SCAN_BLOCK)
#define GS_AS_SLOT 16         // 16-bit words of a line's slot (GS_AS_S_*)
enum { GS_AS_S_START = 0,     // slot: the line's first byte in the chunk (two words)
       GS_AS_S_TABS = 2,      // its tabs
       GS_AS_S_LEN = 3,       // its bytes without the terminator
       GS_AS_S_TAB = 4 };     // nine words: tabs number 4 5 6 7 10 11 12 19 20, as offsets from the line's first byte
enum { GS_AS_BAD_LINE = 0, GS_AS_LONGEST = 1, GS_AS_WORDS = 2 };
enum { GS_AS_C_COUNTED = 0, GS_AS_C_KEPT = 1, GS_AS_C_SHORT = 2, GS_AS_C_SKIPPED = 3, GS_AS_C_POOL = 4, GS_AS_C_WORDS = 6 };  // the chunk's counters
#define GS_AS_KEPT (1ull << 63)  // verdict of a line: kept | is_ref << 40 | quality << 32 | node
struct GsAsmEntry {           // one kept entry, 40 bytes
    int32_t node;
    uint32_t meta;            // quality | is_ref << 8
    int64_t line;             // 0-based, of the whole stream
    unsigned long long pool_off;  // where its three strings lie in the pool, back to back: tax id, species tax id, ftp path
    uint32_t len[3], pad;
};
struct GsAsmsumParams {
    const uint8_t *text;          // n_bytes of whole lines, zero bytes behind them up to n_tiles * GS_AS_TILE + 64
    int64_t n_bytes, n_tiles, n_lines;  // n_lines: newlines, and one more for an unterminated tail
    int32_t last;                 // != 0: the stream ends with this chunk, whose final line need not be terminated
    int32_t key_field;            // 5 or 6
    int32_t quality_mask, reference_only;
    const int32_t *known;         // n_nodes tax ids, ascending
    const uint8_t *filter;        // n_nodes flags, or nullptr
    int32_t n_nodes, pad;
    unsigned long long *tile_lt;  // per tile: newlines | tabs << 32, then their exclusive prefix (gs_launch_scan_blocks)
    uint32_t *tile_tail;          // per tile: (offset of its last newline + 1, 0: none) | tabs behind that newline << 16
    unsigned long long *scan_tot; // [2] the sums: of tile_lt, of line_blk
    uint32_t *status;             // GS_AS_WORDS
    unsigned long long *chunk;    // GS_AS_C_WORDS
    uint16_t *slots;              // n_lines slots of GS_AS_SLOT words
    uint8_t *high;                // n_lines: != 0: a byte from 0x80 on in the line's key field.  Zeroed by the caller
    unsigned long long *verdict;  // n_lines
    unsigned long long *line_blk; // per block of GS_SCAN_BLOCK lines: kept entries | their pool bytes << 32, then the exclusive prefix
    uint32_t *put_line;           // the write pass: per entry of the chunk, its line in the chunk
    GsAsmEntry *entries;          // the write pass: entry_cap of them
    int64_t first_entry, entry_cap, first_line;
    uint8_t *pool;                // pool_cap bytes
    unsigned long long pool_used, pool_cap;
};

// ---- gs_taxtree.hip: nodes.dmp lines -> tree arrays (the taxtree / taxnodes goals)
#define GS_TT_TILE 4096       // bytes per scan block: GS_SCAN_BLOCK threads, 16 bytes each
#define GS_TT_MAX_LINE 4096   // the reference's line buffer: a longer line is split there
#define GS_TT_N_RANKS 40      // C/tax/Rank.java
#define GS_TT_RANK_BYTES 16   // the longest rank name has 15
#define GS_TT_NONE 0xffffffffu
enum { GS_TT_BAD_LINE = 0, GS_TT_LONGEST = 1, GS_TT_WORDS = 2 };
struct GsTaxRanks {
    uint8_t len[GS_TT_N_RANKS];
    uint8_t text[GS_TT_N_RANKS][GS_TT_RANK_BYTES];
};
struct GsTaxScanParams {
    const uint8_t *text;          // n_bytes of whole lines, zero bytes behind them up to n_tiles * GS_TT_TILE + 64
    int64_t n_bytes, n_tiles;
    int32_t last, pad;            // last != 0: the stream ends with this chunk, whose final line need not be terminated
    const GsTaxRanks *ranks;
    unsigned long long *tile_lb;  // per tile: newlines | bars << 32, then their exclusive prefix (gs_launch_scan_blocks)
    uint32_t *tile_tail;          // per tile: (offset of its last newline + 1, 0: none) | bars behind that newline << 16
    unsigned long long *scan_tot; // [1] the sum
    uint32_t *status;             // GS_TT_WORDS
    uint4 *slots;                 // (id, parent, rank ordinal, 0) per line; id 0: a line that yields nothing.  Zeroed by the caller
    int64_t first_line, slot_cap; // the chunk's first line goes to slot first_line (names: its 1-based number in the stream, less one)
    // the names scan (gs_tt_names_kernel)
    const int32_t *taxids;        // n_nodes tax ids, ascending
    int32_t n_nodes, pad2;
    unsigned long long *win;      // per node: the key of the line whose name it has; 0: none (GS_TT_NAME_KEY)
    unsigned long long *name_off; // per node: where its name lies in the pool ...
    uint32_t *name_len;           // ... and its bytes
    uint8_t *pool;                // names of the winners so far, dead ones among them
    unsigned long long *pool_used;
};
// a scientific line with its line number is above every other line; among the others the lower line number is
#define GS_TT_NAME_KEY(scientific, line) ((scientific) ? (1ull << 63) | (unsigned long long)(line) : 0x7fffffffffffffffull - (unsigned long long)(line))
// the node arrays of a finished tree, all on the device, n entries each unless said otherwise
struct GsTaxTreeArrays {
    int32_t n, root;
    const int32_t *taxids;
    int32_t *parent, *rank, *line_of, *depth, *position, *subtree;
    int32_t *node_at;             // node_at[position]: the node, for the nodes the root reaches
    uint8_t *cyc;                 // != 0: the node lies on a cycle of parent links
};
