/*
 * gsgpu.h -- C ABI of the MI355X-native engine for Genestrip's `match` / `filter` hot path.
 *
 * This is the drop-in boundary.  The reference (pure Java) has no FFI for this
 * path; its seams are Java virtual methods.  Each entry point below names the reference interface it
 * replaces (paths relative to /root/reference, C/ = core/src/main/java/org/metagene/genestrip/).
 * INTEGRATION.md shows the JNI stub + Java subclasses a maintainer would add on the reference side.
 *
 * Conventions
 *  - plain C types only; every function returns 0 (GS_OK) or a negative GS_E_* code; the message of the
 *    last failure on the calling thread is available from gs_last_error().  No exceptions cross the ABI.
 *  - arrays passed to *_create are borrowed for the duration of the call (copied to HBM before return).
 *  - handles are not thread safe; use one submitting thread per handle.  Handles on different devices
 *    (one process per GPU) are independent.
 *  - `mem` says where the batch pointers of a submit call live: GS_MEM_HOST (pageable or pinned host
 *    memory; the library stages it to HBM) or GS_MEM_DEVICE (already resident in HBM of the handle's
 *    device; used by bench.py and by callers that ingest on the GPU).  It applies to inputs and outputs.
 *  - every handle works on its own HIP stream.  Device buffers handed to a call must be COMPLETE: the
 *    caller synchronises the stream that produced them first; outputs are complete after the matching
 *    *_sync / *_finish call.  (genestrip_amd/binding.py waits for torch's current stream for you.)
 */
#ifndef GSGPU_H
#define GSGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 3

enum {
    GS_OK = 0,
    GS_E_INVALID = -1,   /* bad argument                                   */
    GS_E_NOMEM = -2,     /* host or device allocation failed               */
    GS_E_HIP = -3,       /* a HIP runtime call failed                      */
    GS_E_UNSUPPORTED = -4,
    GS_E_STATE = -5,     /* call order violated                            */
    GS_E_NODEVICE = -6,  /* no usable gfx950 device                        */
    GS_E_IO = -7,        /* reading or writing a file failed (host layer)  */
    GS_E_CANCELLED = -8  /* a file-level call was stopped on request (gs_host_control, include/gshost.h) */
};

enum { GS_MEM_HOST = 0, GS_MEM_DEVICE = 1, GS_MEM_DEVICE_TEXT = 2 /* gs_match_submit_text / gs_filter_submit_text: the text in HBM, the per-read results to host memory */ };

const char *gs_last_error(void);
const char *gs_strerror(int code);

/* The library keeps the device buffers of finished runs (text banks, queues, result arrays: up to GS_DEVICE_CACHE_MB, default
 * 4096) for the next run of the same shape -- allocating and unmapping them is a fifth of a 30 ms file-level call.  This frees
 * what waits (it is also freed, by itself, when an allocation fails).  The reference has no counterpart: its buffers are JVM heap. */
int gs_device_cache_trim(void);
int gs_abi_version(void);
int gs_device_count(int *n);

/* ---------------------------------------------------------------------------------------------------
 * Device-resident k-mer store + taxonomy
 *
 * Replaces, for lookups: KMerStore.getLong (C/store/KMerSortedArray.java:298-349,
 * C/store/RadixKMerStore.java:369-412) and the SmallTaxTree ancestor/LCA queries
 * (C/tax/SmallTaxTree.java:184-289).  Filled from the Java side through KMerStore.visit
 * (C/store/KMerSortedArray.java:426-439): (kmer, valueIndex) in ascending kmer order.
 *
 *   kmers_sorted[n_entries]  canonical k-mers in the reference encoding (CGAT.java:66-74,145-147), distinct, in
 *                            KMerStore.visit order: ascending for the default KMerSortedArray; by radix bucket and
 *                            remaining bits for the opt-in RadixKMerStore (C/store/RadixKMerStore.java:714-729).
 *                            Any order of distinct k-mers is accepted (ascending input skips the distinctness sort).
 *   value_idx[n_entries]     store value index of each k-mer, in [0, n_values)
 *   parent_vi[n_values]      value index of the parent tree node; -1 for the root; -2 if the value has
 *                            no tree node (Database.convertKMerStore maps it to null => k-mer is a miss,
 *                            C/store/Database.java:136-143).  Every tree node has a value index
 *                            (Database.initStoreIndices, C/store/Database.java:107-128).
 *                            NULL => no tree (classification must be off); every value is a node.
 *
 * The device layout (super-k-mer records, overflow table, minimizer gate: genestrip_amd/csrc/gs_layout.h) is laid out ON the
 * device for stores with records (k >= 19, at most 2^21 values): 473 M k-mers in under a second, the same bytes from the same
 * arrays every time (runs on separately built replicas stay mergeable).  GS_BUILD_HOST=1 selects the host builder, which also
 * serves the other stores.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_db gs_db;

typedef struct {
    int32_t k;
    int32_t n_values;
    int64_t n_entries;      /* entries handed in                                            */
    int64_t n_stored;       /* entries in the device table (reachable + with a tree node)   */
    int64_t n_buckets;      /* 64-byte buckets of 8 slots (table)                           */
    int64_t table_bytes;
    int32_t max_displacement;
    int32_t value_bits;
    int64_t gate_bytes;     /* L2-resident pre-filter (0 = not built: store too large for it)  */
    int64_t mgate_bytes;    /* minimizer gate (0 = not built: k < 19)                           */
    int64_t rec_bytes;      /* super-k-mer records (0 = not built: k < 19, partition, > 2^21 values) */
    int64_t n_in_records;   /* stored k-mers that live in records (the others are table slots)  */
    int32_t n_stripes;      /* striped store: devices the record table is split over (else 0)  */
    int32_t stripe;         /* ... and which stripe this handle's device holds                  */
    int64_t stripe_bytes;   /* ... and its size                                                  */
} gs_db_info;

int gs_db_create(gs_db **out, int device, int k, int64_t n_entries, const int64_t *kmers_sorted,
                 const int32_t *value_idx, int32_t n_values, const int32_t *parent_vi);
int gs_db_get_info(const gs_db *db, gs_db_info *info);
int gs_db_destroy(gs_db *db);

/* Native store file: the built device image (table, gate, taxonomy arrays), so that a later
 * process loads it straight into HBM instead of going through Java deserialisation (Database.load,
 * C/store/Database.java:265-314) + KMerStore.visit + gs_db_create.  Not portable across layout versions. */
int gs_db_save(gs_db *db, const char *path);
int gs_db_load(gs_db **out, int device, const char *path);

/* ---------------------------------------------------------------------------------------------------
 * The store read back (genestrip_amd/csrc/gs_export.hip): KMerStore.visit (C/store/KMerSortedArray.java:426-439),
 * Database.getStats / getFixedNKmersPerTaxid (C/store/Database.java:159, AbstractKMerStore.java:364) and the db2fastq goal
 * (C/goals/DB2FastqGoal.java, C/fastqgen/KMerFastqGenerator.java, FastQWriter.java).  Every record line and table bucket
 * of the handle's store is decoded on the device (the layout is reversible); seen bits are masked, so these calls may run
 * while a unique-counting run is alive on the store.
 *
 * What comes back is the n_stored pairs of the store: the pairs handed to gs_db_create (or built by gs_dbbuild) that are
 * reachable (x >= revcomp(x): the reference only ever looks up max(fwd, revcomp), CGAT.java:145-147) and whose value has a
 * tree node (parent_vi != -2).  The reference's visit also returns the pairs this store drops; nothing can bring those back.
 * A partition store (gs_db_create_part) gives its own part, a stripe its record lines and its share of the table: the union
 * over the parts / stripes is the whole store.
 *
 *   gs_db_value_counts     counts[n_values] (host) = stored k-mers per value index (the `db_kmers` of gs_host_write_csv)
 *   gs_dbexport_create     decode + sort: the selected pairs, ascending by k-mer (KMerSortedArray.visit order).  sel_vi = -1:
 *                          all; else value == sel_vi (with_desc == 0) or the value's node in the subtree of sel_vi (with_desc != 0)
 *   gs_dbexport_fetch      kmers (reference encoding) + value_idx, *n_kmers entries each; mem = GS_MEM_HOST or GS_MEM_DEVICE
 *   gs_dbexport_fastq_*    the pairs as FASTQ text on the device, what FastQWriter prints for KMerFastqGenerator.generateFastq
 *                          (out, taxid, project + ":", withDesc): record i = 1, 2, .. is
 *                          "@GENESTRIP:<project>::<taxids[value]>:<i>\n<k bases>\n+\n<'~' x k>\n" (CGAT.longToKMerStraight).
 *                          _begin takes taxids[n_values] (host; NULL prints as empty) and the project name and rewinds; each
 *                          _next returns the text of the next records in device memory (valid until the next call, at most
 *                          GS_EXPORT_CHUNK_BYTES, default 256 MiB); *n_records = 0: the text is through.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_dbexport gs_dbexport;
int gs_db_value_counts(gs_db *db, int64_t *counts);
int gs_dbexport_create(gs_dbexport **out, gs_db *db, int32_t sel_vi, int with_desc, int64_t *n_kmers);
int gs_dbexport_fetch(gs_dbexport *x, int64_t *kmers, int32_t *value_idx, int mem);
int gs_dbexport_get_device(gs_dbexport *x, int *device);
int gs_dbexport_fastq_begin(gs_dbexport *x, const char *const *taxids, const char *project);
int gs_dbexport_fastq_next(gs_dbexport *x, const uint8_t **d_text, int64_t *n_bytes, int64_t *n_records);
int gs_dbexport_destroy(gs_dbexport *x);

/* ---------------------------------------------------------------------------------------------------
 * match
 *
 * Replaces FastqKMerMatcher.runMatcher / matchRead (C/match/FastqKMerMatcher.java:181-235, :327-535)
 * plus KMerUniqueCounterBits (C/store/KMerUniqueCounterBits.java:117-163).  One gs_run corresponds to
 * one runMatcher call (one output key): stats and the unique bitmap start cleared (:192-193).
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_run gs_run;

typedef struct {
    int32_t classify;           /* taxTree != null (MatchResultGoal.java:125-127)                */
    int32_t count_unique;       /* GSConfigKey countUniqueKMers (C/GSConfigKey.java:305)         */
    int32_t max_paths;          /* maxClassificationPaths (:350), 1..128                         */
    int32_t threshold;          /* minKMersForClass (:341)                                       */
    double max_read_tax_err;    /* maxReadTaxErrorCount (:328), -1 = off                         */
    double max_read_class_err;  /* maxReadClassErrorCount (:337), -1 = off                       */
    int32_t profile;            /* != 0: record HIP events around the kernels of each submit     */
    int32_t max_kmer_res_counts; /* maxKMerResCounts (:344): > 0 keeps per-k-mer hit counters for gs_match_max_counts */
} gs_match_cfg;

/* integer result table: one row per value index (CountsPerTaxid fields, C/match/CountsPerTaxid.java:127-159) */
enum {
    GS_C_READS = 0,
    GS_C_READS_KMERS,
    GS_C_KMERS,
    GS_C_UNIQUE_KMERS,       /* -1 in every row when count_unique == 0 (FastqKMerMatcher.java:226-230) */
    GS_C_CONTIGS,            /* Java field is int; the table keeps the exact 64-bit count               */
    GS_C_CONTIG_LEN_SQ_SUM,
    GS_C_MAX_CONTIG_LEN,
    GS_C_READS_1KMER,
    GS_C_READS_BPS,
    GS_C_MAX_CONTIG_READ_NO, /* readNo of the first read (file order) with the max contig, -1 if none   */
    GS_N_COLS
};
enum { GS_D_ERR_SUM = 0, GS_D_ERR_SQ_SUM, GS_D_CLASS_ERR_SUM, GS_D_CLASS_ERR_SQ_SUM, GS_N_DCOLS };

/* per-read flags (optional output) */
enum {
    GS_F_FOUND = 1,     /* >= 1 k-mer of the read hit the store                                   */
    GS_F_RETURNED = 2,  /* matchRead's return value: read goes to the filtered FASTQ (:304-307)   */
    GS_F_COUNTED = 4    /* read passed the class-error gate and was added to `reads` (:508-526)   */
};

int gs_match_begin(gs_run **out, gs_db *db, const gs_match_cfg *cfg);

/* One batch of reads: read i = seq[offsets[i] .. offsets[i+1]), readNo = first_read_no + i
 * (AbstractFastqReader.java:343).  class_vi / flags may be NULL; when given they receive, per read,
 * entry.classNode's value index (-1 = null) and GS_F_* bits.  Asynchronous for GS_MEM_DEVICE (call
 * gs_match_sync / gs_match_finish before reading outputs); synchronous for GS_MEM_HOST. */
int gs_match_submit(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads,
                    int64_t first_read_no, int mem, int32_t *class_vi, uint8_t *flags);
/* The same for reads of ONE length lying back to back (read i = seq[i * read_len .. (i + 1) * read_len)): no offsets array to
 * build, stage or read -- on the device the offsets' round trip in front of every read's bases is gone.  What a host holds after
 * parsing a sequencer's FASTQ (fixed cycles) and what bench.py's resident reads are. */
int gs_match_submit_fixed(gs_run *run, const uint8_t *seq, int32_t read_len, int64_t n_reads, int64_t first_read_no, int mem,
                          int32_t *class_vi, uint8_t *flags);
int gs_match_sync(gs_run *run);
/* The asynchronous form for HOST batches (the producer thread of AbstractFastqReader fills batch i+1 while batch i is
 * on the device): returns as soon as the work is queued -- for page-locked arrays (gs_pinned_alloc) that is at once,
 * and the copy of this batch runs under the kernel of the previous one -- and hands out a ticket.  gs_match_wait(ticket)
 * returns when class_vi / flags of that batch are filled in and seq / offsets may be reused; at most two batches should
 * be under way (a third submit waits for the first on the device).  gs_match_sync / gs_match_finish wait for all. */
int gs_match_submit_async(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads,
                          int64_t first_read_no, int32_t *class_vi, uint8_t *flags, int64_t *ticket);
int gs_match_wait(gs_run *run, int64_t ticket);

/* Text mode: a chunk of RAW FASTQ text made of whole four-line records; the device finds the records itself
 * (replaces the producer-thread parse of AbstractFastqReader.doReadFastq, C/fastq/AbstractFastqReader.java:288-368,
 * for the common file shape; read i of the chunk is its (4i+2)-th line, '\r' kept, readNo = first_read_no + i).
 * n_lines = number of '\n' in the chunk as counted by the caller: a multiple of 4, the chunk ends with one.
 * The chunk is REFUSED on the device -- nothing of it, nor of any later text chunk, reaches the run's state -- if
 * it is not exactly what the reference would split into one record per four lines: a NUL byte (the reference drops
 * those, B/io/BufferedLineReader.java:176-178), a third line that does not start with '+' (multi-line sequence,
 * :301-308), a quality line shorter than its sequence (:320-341), or a newline count other than n_lines.
 * gs_match_text_status reports the ticket of the first refused chunk (-1: none); the caller re-parses from there
 * with the general parser, calls gs_match_text_clear_error and goes on.  Asynchronous: with GS_MEM_HOST the text
 * must stay untouched until gs_match_text_wait_copy(ticket) returns (use gs_pinned_alloc for overlap); class_vi /
 * flags (n_lines / 4 entries, same memory kind as text, may be NULL) are complete after gs_match_sync.
 * totals[3] = reads, k-mers (sum of max(0, L-k+1)) and bases of all ACCEPTED chunks since begin/reset
 * (AbstractFastqReader.java:343-349).  Chunks are limited to 1 GiB. */
int gs_match_submit_text(gs_run *run, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem,
                         int64_t first_read_no, int32_t *class_vi, uint8_t *flags, int64_t *ticket);
/* The same for FASTA (AbstractFastqReader.doReadFasta, C/fastq/AbstractFastqReader.java:375-438): a chunk of raw FASTA
 * text made of whole records -- it starts with a header line ('>'), ends with a newline, n_lines = its newlines,
 * n_records = its header lines (lines whose first byte is '>'), both counted by the caller.  Read i is the concatenation
 * of the sequence lines of record i ('\r' kept; a record without sequence lines is a read of length 0).  The device finds
 * the records with two prefix sums over the lines and gathers the sequences.  Refused (as above, same status calls) if
 * the counts do not match, the chunk does not start with a header, it holds a NUL byte, or ANY line is empty (there the
 * reference's loop looks at a stale byte of its buffer, :386-392: such input belongs to the reference-exact parser).
 * n_records < 2^24 per chunk.  class_vi / flags: n_records entries. */
int gs_match_submit_fasta(gs_run *run, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int64_t n_records, int mem,
                          int64_t first_read_no, int32_t *class_vi, uint8_t *flags, int64_t *ticket);
/* General FASTQ (AbstractFastqReader.doReadFastq, C/fastq/AbstractFastqReader.java:288-368, with sequence and quality over any
 * number of lines): `text` = whole lines (n_lines newlines, the last byte is one) that START with a record's descriptor line.  The
 * device finds the record structure -- per line where the next record would start if one started here, then the orbit of line 0
 * by pointer doubling -- and matches the records that END inside the chunk; *n_records is their number, *consumed_bytes what they
 * cover (*consumed_lines, may be NULL: their lines): the caller puts the rest in front of the next chunk.  The call waits for the
 * structure (not for the match; the text has been copied when it returns).  A chunk with a NUL byte or a record of more than
 * 4096 lines is refused like a malformed four-line chunk: *n_records = -1, nothing is matched, gs_match_text_status /
 * gs_match_text_clear_error as there. */
int gs_match_submit_fastq_ml(gs_run *run, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, int64_t first_read_no,
                             int32_t *class_vi, uint8_t *flags, int64_t *n_records, int64_t *consumed_bytes, int64_t *consumed_lines,
                             int64_t *ticket);
/* (class_vi / flags: optional per-read outputs as for gs_match_submit_text, room for n_lines / 4 + 1 reads.)  After such a chunk:
 * classes[0 .. consumed_lines) = 1 for a record's descriptor line, 2 for its sequence lines, 0 otherwise; with
 * gs_match_text_newlines this is the record geometry for per-read output. */
int gs_match_text_line_classes(gs_run *run, uint8_t *classes);
int gs_match_text_wait_copy(gs_run *run, int64_t ticket);
int gs_match_text_status(gs_run *run, int64_t *failed_ticket, int64_t *first_bad_record, int64_t totals[3]);
int gs_match_text_clear_error(gs_run *run);
/* Files that are read side by side are independent streams of chunks: a refusal in one must not silence the others.
 * The refusal state and the totals exist in 16 banks; submit / status / clear_error work on the selected one (0 at
 * begin).  Use first_read_no to keep the read numbers of the files apart. */
int gs_match_text_select(gs_run *run, int bank);
/* page-locked host memory for the text blocks (so that the H2D copy overlaps the caller's file reads) */
int gs_pinned_alloc(void **p, size_t bytes);
int gs_pinned_free(void *p);

/* table: n_values x GS_N_COLS int64 ; dtable (may be NULL): n_values x GS_N_DCOLS double (sums of doubles
 * accumulate in device order: not bit-reproducible, as with threads > 0 in the reference).  Host pointers. */
int gs_match_finish(gs_run *run, int64_t *table, double *dtable);
/* The reference copies the read's descriptor whenever a contig beats the current maximum of its tax id
 * (CountsPerTaxid.maxContigDescriptor, FastqKMerMatcher.java:401-407).  A host that cannot keep the descriptors of all
 * reads asks after every batch: read_no[n_values] (host) = read number that currently holds the maximum (-1: none).  A
 * maximum only ever moves to a LATER batch's read by beating it, so the descriptor a host copies when the answer falls
 * into the batch it just submitted is, at the end, the one gs_match_finish reports.  Synchronises. */
int gs_match_max_contig_reads(gs_run *run, int64_t *read_no);
int gs_match_reset(gs_run *run); /* same matcher, next key: clears stats + unique bitmap */
int gs_match_destroy(gs_run *run);

/* maxKMerResCounts > 0 (experimental CSV column "max kmer counts"; KMerUniqueCounterBits.getMaxCountsCounts,
 * C/store/KMerUniqueCounterBits.java:173-211): the `max_kmer_res_counts` largest per-k-mer hit counts of every value
 * index (rows 0..n_values-1) and over all values (row n_values), descending, zero padded; counts are Java shorts
 * (they wrap at 2^15 exactly like `++countsVector.shorts[i]`).  out: (n_values + 1) x max_kmer_res_counts int16, host.
 * Not supported in DB-partitioned mode. */
int gs_match_max_counts(gs_run *run, int16_t *out);

/* Multi-GPU (read-sharded) merge hooks: raw device pointers of the run's accumulators so that the host
 * can reduce them over RCCL before gs_match_finish (sum over ranks for `sums`, max for `max_keys`,
 * all-gather + gs_match_or_bitmap for the unique bitmap).
 *   sums      int64  [n_values][GS_N_SUMS]   additive columns
 *   max_keys  int64  [n_values]              (maxContigLen << 40) | (2^40-1 - readNo), 0 = none
 *   dsums     double [n_values][GS_N_DCOLS]
 *   bitmap    uint32 [bitmap_words]          one bit per table slot                                */
enum { GS_S_READS = 0, GS_S_READS_KMERS, GS_S_KMERS, GS_S_CONTIGS, GS_S_CONTIG_LEN_SQ_SUM, GS_S_READS_1KMER,
       GS_S_READS_BPS, GS_N_SUMS };
int gs_match_device_state(gs_run *run, void **sums, void **max_keys, void **dsums, void **bitmap,
                          int64_t *bitmap_words);
/* bitmap |= OR of n_parts device bitmaps laid out back to back at `parts` (each bitmap_words long) */
int gs_match_or_bitmap(gs_run *run, const void *parts, int64_t n_parts);

/* The same merge for runs that live in ONE process -- what a JVM host does with one gs_run per GPU of the node (the
 * reference is a single process: C/fastq/AbstractFastqReader.java:85-104; it has no counterpart of torch.distributed).
 * Every run must work on a replica of the same store (same arrays through gs_db_create / the same store file).  Runs on
 * the same device are reduced by kernels, the devices among each other by RCCL collectives over xGMI (all-reduce SUM of
 * `sums` / `dsums`, all-reduce MAX of `max_keys`, all-gather + OR of the unique bitmaps; librccl is loaded on first
 * use); the per-k-mer hit counters of runs begun with max_kmer_res_counts > 0 are summed through host memory.  Afterwards
 * EVERY run holds the global state: gs_match_finish and gs_match_max_counts on any of them return what a single run over
 * all the reads would have produced (give the runs disjoint read numbers: first_read_no).  Synchronous. */
int gs_match_merge(gs_run *const *runs, int n_runs);

/* ---------------------------------------------------------------------------------------------------
 * Striped store (BASELINE.json configs[4]: a store that does not fit one GPU).  The super-k-mer
 * record table -- the bulk of a store -- is split into n_stripes runs of consecutive buckets, stripe p in the HBM of one
 * device; gates, overflow table and tree are small and live on every device.  Reads stay on their home GPU and go
 * through the SAME fused kernel as with a replicated store (gs_match_submit* / gs_match_segments): a record line of a
 * foreign stripe is simply loaded over xGMI peer access (64 bytes per minimizer run that passed the gate), there is no
 * exchange step, no materialised key stream and no host synchronisation per batch.  Record lines are never written:
 * the seen bits of a striped store are kept in each run's own bitmap, and gs_match_merge / the torch.distributed merge
 * OR them exactly as for replicas.  With one stripe this IS gs_db_create.  No counterpart in the single-process
 * reference.
 *
 * gs_db_create_striped: all stripes from ONE process (a JVM host with one gs_run per GPU): out[p] = handle on
 *   devices[p] (2..8 devices that can access each other; a device may appear more than once, which puts several stripes
 *   on it -- how the tests rehearse this on one GPU).  The stripes are freed with the last of the handles.
 * gs_db_create_stripe: ONE stripe per process (torch.distributed, one process per GPU): every process builds the layout
 *   from the same arrays and keeps stripe `stripe`; then every process exports its stripe (gs_db_stripe_export: 64 opaque
 *   bytes, a HIP IPC memory handle), the hosts exchange them (all-gather), and each attaches the others
 *   (gs_db_stripe_attach).  gs_match_begin refuses a handle whose stripes are not all attached.  The exporting process
 *   must keep its handle alive while others use the stripe.
 * ------------------------------------------------------------------------------------------------- */
#define GS_MAX_STRIPES 8
#define GS_STRIPE_HANDLE_BYTES 64
int gs_db_create_striped(gs_db **out, const int *devices, int n_stripes, int k, int64_t n_entries, const int64_t *kmers,
                         const int32_t *value_idx, int32_t n_values, const int32_t *parent_vi);
int gs_db_create_stripe(gs_db **out, int device, int n_stripes, int stripe, int k, int64_t n_entries, const int64_t *kmers,
                        const int32_t *value_idx, int32_t n_values, const int32_t *parent_vi);
int gs_db_stripe_export(gs_db *db, void *handle);
int gs_db_stripe_attach(gs_db *db, int stripe, const void *handle);
/* The same from a store file (gs_db_save of the store built ONCE by gs_db_create): nobody rebuilds the layout, every process
 * reads the image, checks it as gs_db_load does and keeps its stripe.  The usual way to bring a big store up. */
int gs_db_load_striped(gs_db **out, const int *devices, int n_stripes, const char *path);
int gs_db_load_stripe(gs_db **out, int device, int n_stripes, int stripe, const char *path);

/* ---------------------------------------------------------------------------------------------------
 * DB construction: the compute core of FillDBGoal + DBGoal -- every k-mer of every genome region of
 * the requested taxa is stored under its tax node (C/goals/refseq/FillDBGoal.java:297ff -> KMerSortedArray.putLong,
 * C/store/KMerSortedArray.java:168-202: the first region that holds a k-mer sets its value), then every region of the whole
 * reference collection updates the k-mers it shares with the store to the lowest common ancestor of the old value and its own
 * node (C/goals/refseq/DBGoal.java:233-256, :299-311 -> KMerStore.update, TaxTree.getLowestCommonAncestor,
 * C/tax/TaxTree.java:160-187).  K-mers are formed as AbstractStoreFastaReader.dataLine does (C/refseq/
 * AbstractStoreFastaReader.java:87-115 over C/util/CGATLongBuffer.java:137-229): per region a window of the last k bases,
 * reset by any byte that is not C, G, A, T (after upper-casing a, c, g, t if lower_case_bases: GSConfigKey lowerCaseBases,
 * default on), taken when (bases of the region so far) % step_size == 0, stored as CGAT.standardKMer.
 *
 *   gs_dbbuild_begin   tree as for gs_db_create (parent_vi: -1 the ONE root, -2 no node); max_dust = GSConfigKey maxDust (-1 off):
 *                      k-mers whose low-complexity score (CGATLongBuffer.getDustValue, the sum of fib(run length) over the runs of
 *                      period 1, 2 and 3 inside the k-mer) exceeds it are skipped in both passes (:105-107).
 *   gs_dbbuild_add     regions = FASTA records without their header and line ends (seq, offsets[n_regions + 1], offsets[0] = 0;
 *                      `mem` says where seq / offsets live), node_vi[n_regions] (host) = value index of each region's node
 *                      (FillDBGoal / DBGoal reworkNode: the host's mapping).  update = 0: a FillDBGoal region (its k-mers are
 *                      stored), update = 1: a DBGoal region (only LCA updates).  Regions count in the order they are added.
 *   gs_dbbuild_finish  one stable radix sort of all (k-mer, region) pairs + one pass over the runs of equal k-mers.
 *   gs_dbbuild_fetch   kmers ascending (the reference's encoding) + value_idx: the arrays gs_db_create takes.
 *
 * Differences to the reference, all of them run-to-run variations of the reference itself: putLong drops a new k-mer
 * when the fill Bloom filter reports a false positive (:175-186) -- which k-mers depends on the insertion order of its
 * reader threads -- and with several reader threads "first" is a race; here every k-mer of a fill region is stored and the
 * first region in the order of the add calls wins.  maxKMersPerTaxid / maxGenomesPerTaxid / a full store (:187-190) are the
 * host's business (they decide which regions are handed in).
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_dbbuild gs_dbbuild;
int gs_dbbuild_begin(gs_dbbuild **out, int device, int k, int32_t n_values, const int32_t *parent_vi, int lower_case_bases, int max_dust,
                     int step_size);
int gs_dbbuild_add(gs_dbbuild *b, const uint8_t *seq, const uint64_t *offsets, const int32_t *node_vi, int64_t n_regions, int mem,
                   int update);
/* A collection whose pairs do not fit the GPU (40 bytes per genome base at the peak) is built in passes over disjoint ranges of
 * the canonical k-mer: before the first gs_dbbuild_add, keep only the k-mers in [lo, hi); hand the same regions to one builder
 * per range; the results of ascending ranges, one behind the other, are the result of a single build.  (Canonical k-mers are
 * the larger of two strands, so equal shares of the k-mers lie between 4^k * sqrt(i / n): genestrip_amd.binding.kmer_ranges.) */
int gs_dbbuild_set_range(gs_dbbuild *b, uint64_t lo, uint64_t hi);
int gs_dbbuild_finish(gs_dbbuild *b, int64_t *n_kmers);
int gs_dbbuild_fetch(gs_dbbuild *b, int64_t *kmers, int32_t *value_idx);
/* ... or straight into a store on the builder's device, without the arrays ever leaving the GPU: genomes -> gs_dbbuild_add ->
 * gs_dbbuild_finish -> gs_dbbuild_to_db -> gs_match_begin (and gs_db_save for later processes).  Every k-mer of the build must
 * be reachable, which it is by construction (canonical k-mers).  Stores without records: GS_E_UNSUPPORTED (fetch + gs_db_create). */
int gs_dbbuild_to_db(gs_dbbuild *b, gs_db **out);
int gs_dbbuild_destroy(gs_dbbuild *b);

/* ---------------------------------------------------------------------------------------------------
 * Store quality against its source genomes (genestrip_amd/csrc/gs_quality.hip): the compute core of the reference's
 * dbqualcounts goal (ft/src/main/java/org/metagene/genestrip/finertree/goals/DBQualityCountsGoal.java, MyFastaReader.handleStore
 * :250-289 and doMakeThis :137-147).  The genomes are walked again and every k-mer is looked up in the finished store; per
 * leaf value index three counts come back:
 *   tp      distinct k-mers of the leaf's genomes that are stored under the leaf's node or one of its ancestors
 *   tp+fp   all k-mers stored on the path leaf -> root (the sum of gs_db_value_counts over that path)
 *   tp+fn   distinct k-mers of the leaf's genomes that are stored at all (under a value that has a tree node)
 * precision = tp / (tp+fp), recall = tp / (tp+fn) (gs_host_write_quality_csv, include/gshost.h).
 *
 *   gs_dbquality_begin      k, n_values and the tree are the store's; lower_case_bases / max_dust / step_size as for gs_dbbuild_begin:
 *                           k-mers are formed exactly as there.  The store must stay alive until gs_dbquality_destroy.  A stripe
 *                           of a striped store (gs_db_create_stripe, _striped, gs_db_load_stripe, _striped): GS_E_UNSUPPORTED.  A
 *                           partition store (gs_db_create_part) is taken as the store it is: the counts are those of its part
 *                           (tp and tp+fn of all parts add up to the whole store's).
 *   gs_dbquality_add        regions as for gs_dbbuild_add (seq, offsets[n_regions + 1], `mem`); leaf_vi[n_regions] (host) = value
 *                           index of each region's leaf node, the host's resolution of AbstractUpdateFastaReader.updateLeafNode
 *                           (id node, file node or data child, else the tax node; an inner node of the tree is as good as a
 *                           leaf).  leaf_vi < 0 or a value without a node (parent_vi == -2): the region counts nothing
 *                           (leafNode == null).  leaf_vi >= n_values: GS_E_INVALID.  No work on the store here.
 *   gs_dbquality_finish     sorts the (k-mer, leaf) pairs, joins the distinct ones with the store in ascending k-mer order (decoded
 *                           on the device once per handle, as gs_dbexport_create does) and counts.  counts[n_values][3] = tp,
 *                           tp+fp, tp+fn and present[n_values] (both host): a leaf with tp+fn > 0 has present = 1 and its three
 *                           counts; every other row is absent (the reference's map has no entry): 0, 0, 0 and present = 0.
 *                           The pairs' device memory is released here; the decoded store at gs_dbquality_destroy.
 *   gs_dbquality_set_range  as gs_dbbuild_set_range: before the first gs_dbquality_add of a pass, keep only the canonical k-mers in
 *                           [lo, hi).  tp and tp+fn are additive over disjoint ranges (the pairs partition by k-mer): a collection
 *                           whose pairs do not fit the GPU (24 bytes per genome base at the peak) runs range by range and the
 *                           caller adds the tp / tp+fn columns.  tp+fp does not depend on the range; it is filled for the leaves
 *                           with tp+fn > 0 in THAT range.  Called after gs_dbquality_finish it starts the next pass on the same
 *                           handle, which keeps the decoded store; without it a finished handle takes no further add or finish
 *                           (GS_E_STATE).
 *   gs_dbquality_get_stats  sizes and wall-clock phase times of the latest pass (tools/db_quality_rate.py).
 *
 * One difference to the reference: it removes duplicate (k-mer, leaf) pairs with an XOR Bloom filter (XORKMerIndexBloomFilter,
 * ftBloomFilterFpp), so a false positive silently drops a pair that was never counted -- which pairs depends on the insertion
 * order of its reader threads.  Here de-duplication is exact (sort + heads of runs): the result is the reference's at
 * fpp -> 0, and it is deterministic.  (Compare the builder's note on putLong above.)  The store is only read, and seen bits are
 * masked as in the export: these calls may run while a unique-counting run is alive on the store.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_dbquality gs_dbquality;
typedef struct {
    int64_t n_pairs;    /* (k-mer, leaf) pairs enumerated in this pass                      */
    int64_t n_distinct; /* distinct pairs of the leaves that count                          */
    int64_t n_found;    /* ... whose k-mer is stored (the sum of the tp+fn column)          */
    int64_t n_store;    /* k-mers of the decoded store                                      */
    double ms_pairs;    /* gs_dbquality_add calls of this pass (copy + k-mer kernel)        */
    double ms_sort;     /* leaf sort + k-mer sort                                           */
    double ms_decode;   /* store decode + sort + per-value counts (paid by the first pass)  */
    double ms_join;     /* join + classify + count                                          */
} gs_dbquality_stats;
int gs_dbquality_begin(gs_dbquality **out, gs_db *db, int lower_case_bases, int max_dust, int step_size);
int gs_dbquality_set_range(gs_dbquality *q, uint64_t lo, uint64_t hi);
int gs_dbquality_add(gs_dbquality *q, const uint8_t *seq, const uint64_t *offsets, const int32_t *leaf_vi, int64_t n_regions, int mem);
int gs_dbquality_finish(gs_dbquality *q, int64_t *counts, uint8_t *present);
int gs_dbquality_get_stats(gs_dbquality *q, gs_dbquality_stats *out);
int gs_dbquality_destroy(gs_dbquality *q);

/* ---------------------------------------------------------------------------------------------------
 * A finished store updated in batches (genestrip_amd/csrc/gs_update.hip): the reference's updatedb stage in its own shape.
 * DBGoal.MyFastaReader (C/goals/refseq/DBGoal.java:233-311) streams every region of the whole reference collection past the
 * store that filldb / tempdb left behind; every stored k-mer that occurs in a region gets
 *   value := LCA(value, node of the region)          (:240-254 -> KMerStore.update, TaxTree.getLowestCommonAncestor,
 *                                                     C/tax/TaxTree.java:160-187)
 * and a stored value without a tree node stays as it is (lastLCA = lcaNode != null ? ... : oldValue, :246-251).  gs_dbbuild
 * folds fill and update into one sort, which keeps every pair resident (40 bytes per genome base at the peak) and takes
 * updates only before its own finish.  Here the memory is the store (16 bytes per k-mer + the directory) plus one slice of
 * input (13 bytes per base of the slice), whatever the size of the collection, and the store may come from anywhere.  LCA is
 * associative, commutative and idempotent: the result does not depend on the order or the grouping of the add calls, and adding
 * a region twice changes nothing.  The k-mer array never changes (no k-mer is added to a finished store).
 *
 *   gs_dbupdate_begin        the arrays of gs_dbbuild_fetch / gs_db_create: kmers ascending and distinct in the reference's
 *                            encoding, value_idx in [0, n_values), both in host or device memory (`mem`); they are copied.  One
 *                            device pass checks order, distinctness and ranges: GS_E_INVALID.  Tree, lower_case_bases, max_dust,
 *                            step_size as for gs_dbbuild_begin (forests: GS_E_UNSUPPORTED): k-mers are formed by the builder's own
 *                            kernel.  Every argument is checked before a device is touched.
 *   gs_dbupdate_begin_db     the k-mers of a live store, decoded on the device as gs_dbexport_create does (seen bits masked); k,
 *                            n_values and the tree are the store's.  The store is only read and may be destroyed after the call.
 *                            A stripe of a striped store: GS_E_UNSUPPORTED.  A partition store (gs_db_create_part) is taken as
 *                            the part it is: its k-mers are updated, the other parts' are not there.
 *   gs_dbupdate_begin_build  the result arrays of a builder whose gs_dbbuild_finish has succeeded (else GS_E_STATE), copied device
 *                            to device; the builder's k, tree, lower_case_bases, max_dust and step_size are inherited.  The
 *                            builder stays valid and keeps answering gs_dbbuild_fetch / _to_db with its own, un-updated arrays.
 *   gs_dbupdate_add          regions and node_vi as for gs_dbbuild_add(..., update = 1).  A node_vi that is not a node of the tree,
 *                            or bad offsets: GS_E_INVALID, and the handle is as it was before the call.  The batch is worked off in
 *                            slices of at most max_bases bases (gs_dbupdate_set_slice; default 2^25); a region that is longer
 *                            is cut at multiples of step_size and consecutive pieces overlap by k - 1 bases, so that every window
 *                            is formed exactly once and (bases of the region so far) % step_size counts from the region's start.
 *                            Returns when the caller's arrays are free again.  The working memory of the call is allocated before
 *                            any of its work: GS_E_NOMEM leaves the values as they were before the call.  Any other device error
 *                            in the middle of a call marks the handle failed: every later add / finish / fetch is GS_E_STATE.
 *   gs_dbupdate_set_slice    k - 1 + step_size <= max_bases <= 2^31, else GS_E_INVALID.  Slices do not change any result.
 *   gs_dbupdate_finish       *n_moved = the stored k-mers whose value differs from the value at begin.  This is deterministic;
 *                            the reference's getKMersMoved (C/store/AbstractKMerStore.java:237, logged at DBGoal.java:132) counts move EVENTS instead, which depends on the
 *                            order of the regions (a value that climbs twice counts twice there, once here).  Afterwards the handle
 *                            takes no further add (GS_E_STATE); a second finish repeats the count.
 *   gs_dbupdate_fetch        kmers / value_idx (host, n_store entries: gs_dbupdate_get_stats) -- before finish: GS_E_STATE.
 *   gs_dbupdate_to_db        the arrays into the device layout builder, as gs_dbbuild_to_db: nothing leaves the GPU.  Stores
 *                            without records: GS_E_UNSUPPORTED (fetch + gs_db_create).  Before finish: GS_E_STATE.
 *   gs_dbupdate_get_stats    counts so far and phase times (tools/db_update_rate.py).  batch_bytes_peak depends on the largest slice
 *                            so far, never on the number of add calls.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_dbupdate gs_dbupdate;
typedef struct {
    int64_t n_store;      /* k-mers of the store being updated                                   */
    int64_t n_pairs;      /* (k-mer, region) pairs enumerated so far                             */
    int64_t n_found;      /* ... whose k-mer is stored                                           */
    int64_t n_moved;      /* stored k-mers whose value now differs from the value at begin       */
    int64_t store_bytes;  /* device bytes that live as long as the handle (k-mers, values, index) */
    int64_t batch_bytes_peak; /* largest device footprint of one slice's working memory          */
    double ms_begin, ms_kmers, ms_lookup, ms_finish;
} gs_dbupdate_stats;
int gs_dbupdate_begin(gs_dbupdate **out, int device, int k, int32_t n_values, const int32_t *parent_vi, int lower_case_bases, int max_dust,
                      int step_size, const int64_t *kmers, const int32_t *value_idx, int64_t n_kmers, int mem);
int gs_dbupdate_begin_db(gs_dbupdate **out, gs_db *db, int lower_case_bases, int max_dust, int step_size);
int gs_dbupdate_begin_build(gs_dbupdate **out, gs_dbbuild *finished_builder);
int gs_dbupdate_set_slice(gs_dbupdate *u, int64_t max_bases);
int gs_dbupdate_add(gs_dbupdate *u, const uint8_t *seq, const uint64_t *offsets, const int32_t *node_vi, int64_t n_regions, int mem);
int gs_dbupdate_finish(gs_dbupdate *u, int64_t *n_moved);
int gs_dbupdate_fetch(gs_dbupdate *u, int64_t *kmers, int32_t *value_idx);
int gs_dbupdate_to_db(gs_dbupdate *u, gs_db **out);
int gs_dbupdate_get_stats(gs_dbupdate *u, gs_dbupdate_stats *out);
int gs_dbupdate_destroy(gs_dbupdate *u);

/* ---------------------------------------------------------------------------------------------------
 * A genome collection sized before it is built (genestrip_amd/csrc/gs_size.hip): the two walks the reference makes in front of
 * filldb, on the device.
 *   fillsize   (C/goals/refseq/FillSizeGoal.java:80-105 over C/refseq/AbstractStoreFastaReader.java:87-115): the k-mers of the
 *              collection with duplicates, how many of them the low-complexity gate drops (dustCounter), how many remain
 *   tempindex  (C/goals/refseq/FillBloomFilterGoal.java:154-195, :260-271): the DISTINCT k-mers, in total and per radix bucket
 *              (RadixKMerStore.radixOf = the low radixStoreBits bits); C/goals/refseq/FillDBGoal.java:107-117 sizes its store
 *              from this DBSize
 * and, for this library's own builder, a histogram of the canonical k-mer's top bits from which the passes of a build that does
 * not fit the GPU are planned (the builder's set_range call, gs_dbsize_plan below) instead of guessed.
 *
 * K-mers are formed exactly as the builder's add call forms them (the "DB construction" section above; lower_case_bases /
 * max_dust / step_size as for its begin).  For the bases b[0..len) of a region after the optional upper-casing, the window
 * [s, s + k) counts iff all k bytes are C, G, A or T and (s + k) % step_size == 0.  For every counting window:
 *   total += 1;
 *   if max_dust >= 0 and the window's score exceeds it: dust += 1 and nothing else;
 *   otherwise included += 1, per_value[tag of the region] += 1 and hist[canon >> (2k - hb)] += 1, canon = CGAT.standardKMer of the
 *   window, hb = min(hist_bits, 2k); a handle that keeps keys retains canon as well if lo <= canon < hi.
 * `included` is the number FillSizeGoal sets; total and dust are what it logs as the dust ratio.  Counts and histogram always
 * cover the whole key space: the range restricts only what is retained.  All counters are 64-bit sums over the add calls of the
 * current pass; they depend neither on how the collection is cut into batches nor on `mem`.
 *
 *   gs_dbsize_begin      n_values = number of tags (per_value's length; a caller without tax ids passes 1); the handle takes no
 *                        tree.  max_dust has no upper limit here (the builder's begin refuses values above Short.MAX_VALUE
 *                        with the reference; a score can exceed it -- (AC)^15 A scores fib(29) = 832040 -- and a sizing pass
 *                        may ask what a gate at such a score would drop).  hist_bits 1 .. 12.  radix_bits 0 (no bucket sizes) or 16 .. 24 (GSConfigKey.RADIX_STORE_BITS).
 *                        keep_keys = 0: the pure counting handle -- its device memory is the staged batch plus the counter
 *                        block, and gs_dbsize_distinct answers GS_E_STATE.  Without a GPU: GS_E_NODEVICE.
 *   gs_dbsize_add        regions as for the builder's add call (seq, offsets[n_regions + 1], `mem`); tag_vi[n_regions] (host) = a
 *                        value index in [0, n_values) per region, anything else: GS_E_INVALID and nothing changes.  The memory
 *                        of the call is allocated before any of its work: GS_E_NOMEM leaves the handle as it was.  Any other
 *                        device error marks the handle failed: every later call but destroy is GS_E_STATE.
 *   gs_dbsize_counts     t, per_value[n_values] and hist[1 << hb] (host; per_value and hist may be NULL) of the pass so far.
 *   gs_dbsize_distinct   sorts the retained keys (rocPRIM radix sort over 2k bits) and counts the heads of runs into *n_distinct;
 *                        each head adds one to bucket_sizes[key & (2^radix_bits - 1)] (host, 1 << radix_bits entries; ignored
 *                        when radix_bits = 0).  Distinct counts and bucket sizes are additive over disjoint ranges.  The
 *                        retained keys are released here; no add follows in this pass.
 *   gs_dbsize_set_range  before the first add: the range [lo, hi) of the first pass.  After a counts or distinct call it starts the
 *                        next pass on the same handle and clears every counter.  Any other order: GS_E_STATE.
 *   gs_dbsize_get_stats  sizes and phase times of the pass (tools/db_size_rate.py).  bytes_peak is what the retained keys cost at
 *                        the peak: 8 bytes per key slot (one slot per base of the batch being added, plus up to half again while
 *                        the buffer grows over several add calls) + 8 bytes per retained key for the sort's second buffer + the
 *                        sort's temporary storage -- 16 bytes per key when the pass is one add call, against the builder's 40.
 *   gs_dbsize_plan       host arithmetic, needs no device: ranges for the set_range calls from a histogram.  bounds[0 .. *n_ranges]
 *                        are bin boundaries, bounds[i] = bin << (2k - hb), bounds[0] = 0, bounds[*n_ranges] = 4^k, strictly
 *                        increasing; range i is [bounds[i], bounds[i + 1]).  The ranges are maximal greedy runs of consecutive bins
 *                        whose histogram sum is <= max_pairs (for a contiguous partition under a cap also the fewest); empty bins
 *                        join a neighbour, an all-zero histogram gives one range.  A single bin above max_pairs: GS_E_INVALID,
 *                        the message names the bin and its count (the cure is more hist_bits); more than `cap` ranges (bounds
 *                        holds cap + 1 entries): GS_E_INVALID.  Histograms are additive: a caller who builds fill and update
 *                        regions adds the two arrays before planning.  max_pairs = the device memory the caller grants / 40 for
 *                        the builder, / 24 for the quality pass, / (bytes_peak per key) for the distinct pass.
 *
 * One difference to the reference: FillBloomFilterGoal counts a k-mer as new when its temporary Bloom filter does not hold it
 * yet, and divides the result by (1 - tempBloomFilterFpp) to make up for false positives; which k-mers are miscounted depends
 * on the order of its reader threads.  Here the count is exact (sort + heads of runs): it is the reference's DBSize(size,
 * bucketSizes) at tempBloomFilterFpp -> 0, needs no correction, and is deterministic.  (Compare the quality section's note on
 * its Bloom filter.)  maxKMersPerTaxid / maxGenomesPerTaxid stay the host's business, as in the builder: per_value is what that
 * business needs.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_dbsize gs_dbsize;
typedef struct {
    int64_t total;    /* counting windows                                        */
    int64_t dust;     /* ... dropped by the low-complexity gate (dustCounter)    */
    int64_t included; /* ... that remain: what FillSizeGoal sets                 */
} gs_dbsize_totals;
typedef struct {
    int64_t n_bases;          /* bases handed in during this pass                                    */
    int64_t n_regions;        /* regions handed in during this pass                                  */
    int64_t n_keys;           /* keys retained in this pass                                          */
    int64_t n_distinct;       /* distinct keys of this pass (after the distinct call)                */
    int64_t bytes_fixed;      /* counter block + bucket array: lives as long as the handle           */
    int64_t batch_bytes_peak; /* largest staged batch (bases, offsets, tags)                         */
    int64_t bytes_peak;       /* largest footprint of the retained keys with their sort buffers      */
    double ms_add;            /* add calls of this pass, wall clock (copy + kernel)                  */
    double ms_count;          /* ... the counting kernel alone (device events)                       */
    double ms_sort, ms_heads; /* the distinct call's phases                                          */
    int32_t n_values;         /* entries of per_value                                                */
    int32_t hist_bins;        /* entries of hist: 1 << min(hist_bits, 2k)                            */
    int32_t radix_bits;       /* bucket_sizes holds 1 << radix_bits entries; 0: none                 */
    int32_t keep_keys;
} gs_dbsize_stats;
int gs_dbsize_begin(gs_dbsize **out, int device, int k, int32_t n_values, int lower_case_bases, int max_dust, int step_size, int hist_bits,
                    int radix_bits, int keep_keys);
int gs_dbsize_set_range(gs_dbsize *s, uint64_t lo, uint64_t hi);
int gs_dbsize_add(gs_dbsize *s, const uint8_t *seq, const uint64_t *offsets, const int32_t *tag_vi, int64_t n_regions, int mem);
int gs_dbsize_counts(gs_dbsize *s, gs_dbsize_totals *t, int64_t *per_value, int64_t *hist);
int gs_dbsize_distinct(gs_dbsize *s, int64_t *n_distinct, int64_t *bucket_sizes);
int gs_dbsize_get_stats(gs_dbsize *s, gs_dbsize_stats *out);
int gs_dbsize_destroy(gs_dbsize *s);
int gs_dbsize_plan(const int64_t *hist, int hist_bits, int k, int64_t max_pairs, uint64_t *bounds, int cap, int *n_ranges);

/* ---------------------------------------------------------------------------------------------------
 * DB-partitioned match, the split pipeline of round 1 (kept: it also serves stores without records): the store is split
 * over the GPUs of a node by key hash (gs_db_create_part keeps the keys with (h >> 40) % n_parts == part, h = the library's mixed key), reads stay
 * on their home GPU.  Per batch: gs_match_encode (reads -> h of every k-mer position; ~0 marks a window with a
 * non-CGAT base) -> all-to-all of the keys to their owners -> gs_match_probe_keys on the owner (node = value index,
 * -1 miss, -2 invalid; marks unique k-mers in the owner's table) -> all-to-all back -> gs_match_reduce on the home
 * GPU (the per-read state machine over the node stream).  Unique-k-mer counts of the partitions are disjoint and
 * simply add up.  pos_off[n_reads+1] = exclusive prefix of max(0, L-k+1).  All pointers are DEVICE pointers; the
 * calls are asynchronous on the run's stream (gs_match_sync).  No counterpart in the single-process reference.
 * ------------------------------------------------------------------------------------------------- */
int gs_db_create_part(gs_db **out, int device, int k, int64_t n_entries, const int64_t *kmers_sorted,
                      const int32_t *value_idx, int32_t n_values, const int32_t *parent_vi, int n_parts, int part);
int gs_match_encode(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads, const uint64_t *pos_off,
                    uint64_t *keys);
int gs_match_probe_keys(gs_run *run, const uint64_t *keys, int64_t n_keys, int32_t *nodes);
/* gs_match_encode + gs_route_keys in one pass, without the 8-byte key per k-mer position in between: the keys of owner o
 * go to send_keys[o * cap ..), send_idx holds their position in the batch (~0: a slot that was handed out to a wave but
 * not used -- its key is the invalid-window sentinel, the owner answers it with -2 and gs_unroute_region skips it); the
 * waves take slots 2048 at a time, so counts[o] (HOST array, slots handed out for owner o) is a multiple of 2048 and at
 * most cap; `nodes` receives the node of every position that is NOT routed (the routed ones are overwritten by
 * gs_unroute_region).  cap: a multiple of 2048; *overflow != 0: some region was too small, nothing of the batch may be
 * used (call gs_match_encode + gs_route_keys instead).  Synchronous. */
int gs_match_encode_route(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads, const uint64_t *pos_off,
                          int n_parts, int64_t cap, uint64_t *send_keys, uint32_t *send_idx, int32_t *nodes, int64_t *counts,
                          int *overflow);
/* What a caller needs to size `cap`: the waves gs_match_encode_route launches for a batch of n_reads reads on this run's device
 * (each may leave one chunk partly used per owner) and the chunk size in slots (2048).  No device work. */
int gs_match_route_geometry(const gs_run *run, int64_t n_reads, int32_t *n_waves, int32_t *chunk);
/* nodes[idx[i]] = back[i] for the n answers of one owner region (idx ~0 skipped); asynchronous on the run's stream */
int gs_unroute_region(gs_run *run, const uint32_t *idx, const int32_t *back, int64_t n, int32_t *nodes);
int gs_match_reduce(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads, int64_t first_read_no,
                    const uint64_t *pos_off, const int32_t *nodes, int32_t *class_vi, uint8_t *flags);
/* Routing helpers around the two all-to-alls (device counting sort by owner rank, synchronous):
 * gs_route_keys groups the valid keys by owner: send_keys[n_valid] (owner 0 first), idx[n_valid] = position of each
 * routed key in `keys`, counts[n_parts] (HOST array) = keys per owner; nodes (may be NULL): the positions that are
 * NOT routed get their node right here -- -2 (invalid window, key ~0) or -1 (key ~0 - 1: gs_match_encode found that
 * the store's minimizer gate, which every partition builds over the keys of ALL partitions, rules the k-mer out, so it
 * is a miss without asking its owner).  gs_unroute_nodes scatters the returned nodes back: nodes[idx[i]] = back[i];
 * with keys != NULL it first writes the unrouted positions as above (keys = NULL: gs_route_keys has done it).
 * n_keys < 2^32, n_parts <= 64. */
int gs_route_keys(gs_run *run, const uint64_t *keys, int64_t n_keys, int n_parts, uint64_t *send_keys, uint32_t *idx,
                  int64_t *counts, int32_t *nodes);
int gs_unroute_nodes(gs_run *run, const uint64_t *keys, const uint32_t *idx, const int32_t *back, int64_t n_routed,
                     int32_t *nodes, int64_t n_keys);

/* Kraken-style per-read segments (writeKrakenStyleOut; FastqKMerMatcher.printKrakenStyleOut, :597-611): the maximal
 * runs of equal tax node over the k-mer positions of each read, in read order.  gs_match_segments probes the batch,
 * fills seg_off[n_reads+1] (host array, exclusive prefix of the per-read segment counts) and keeps the segments on
 * the device; gs_match_segments_fetch copies them out: codes[i] = value index, -1 (miss, printed "0") or -2
 * (window with a non-CGAT base, printed "A"), starts[i] = first k-mer position of the run; a run ends where the
 * next one starts (or at L-k+1).  Does not touch the run's statistics.  Outputs are host pointers. */
int gs_match_segments(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads, int mem,
                      uint64_t *seg_off);
int gs_match_segments_fetch(gs_run *run, int32_t *codes, int32_t *starts);
/* the same for the reads of the most recent text chunk (gs_match_submit_text; it must not have been refused), and the
 * byte offsets of that chunk's newlines (n_lines entries, host memory) -- the record geometry a caller needs to write
 * the filtered FASTQ and the Kraken-style lines from its copy of the raw text.  Both synchronise. */
int gs_match_segments_text(gs_run *run, uint64_t *seg_off);
int gs_match_text_newlines(gs_run *run, uint32_t *newlines);
/* ... and the descriptor LINES (the '@' included) of n of that chunk's records (0-based in the chunk), each into `stride` bytes of
 * host memory, NUL-terminated, cut to fit: what a host that never sees the reads needs for CountsPerTaxid.maxContigDescriptor
 * (C/match/FastqKMerMatcher.java:401-407) once gs_match_max_contig_reads has named the reads.  Synchronises. */
int gs_match_text_descriptors(gs_run *run, const int64_t *records, int32_t n, uint8_t *out, int32_t stride);
/* After a FASTA or general-FASTQ chunk: bounds[0 .. n_records] of its reads in the gathered sequence buffer, i.e. the read
 * lengths (bounds[r + 1] - bounds[r]); waits for the chunk. */
int gs_match_text_read_bounds(gs_run *run, uint64_t *bounds);

/* accumulated device time of the match kernel launches since gs_match_begin (cfg.profile != 0) */
int gs_match_kernel_time(gs_run *run, int64_t *launches, double *total_ms);

/* The sampled 15-mer prefilter in front of batches of one read length (gs_match_submit_fixed, 128 .. k + 127 bases): a read none
 * of whose sampled 15-mers occurs in a stored k-mer holds no stored k-mer and is kept off the match kernel.  The filter is a
 * function of the store alone, built on the device by the first run on a store whose density allows it, and never part of the
 * store file; results do not depend on it.  GS_PREFILTER=0 / 1 in the environment (read by gs_match_begin) forces it off / on.
 * info[0]: 1 if the run's store holds a filter; info[1]: distinct canonical 15-mers of the store (-1: never counted);
 * info[2], info[3]: survivors and reads of the last submitted batch (survivors -1: it went without the prefilter).  Synchronises. */
int gs_match_prefilter_info(gs_run *run, int64_t *info);
/* In such a batch on a store whose counters live in LDS (at most 128 values) the match kernel only looks k-mers up.  A read without a
 * non-CGAT byte whose hit k-mers all carry one tax id leaves it as a 32-byte record of its hit positions; a read of several tax ids
 * or with a non-CGAT byte leaves it as the node of every k-mer position (256 bytes).  Two kernels behind it turn both into contigs,
 * classification and counters, one lane per read; results do not depend on it.  GS_SN_DEFER=0 / 1 in the environment (read by
 * gs_match_begin) forces it off / on; the default is on.  Off, such a batch goes through the kernel's general loop.
 * info[0]: 1 if the last submitted batch went this way; info[1]: the records of reads of one tax id it booked; info[2]: the reads
 * that left as nodes per position (both 0 when info[0] is 0).  info holds three values.  Synchronises. */
int gs_match_sn_info(gs_run *run, int64_t *info);
/* Reads that passed the prefilter skip the minimizer gate: for a read from the store the gate passes nearly every k-mer, so a batch
 * behind the prefilter (or one the prefilter's feedback rule sends past it) on a store whose predicted pass probability of a random
 * read is small goes through a loop of the match kernel that never asks the gate; results do not depend on it.  GS_PF_GATE=1 / 0 in
 * the environment (read by gs_match_begin) keeps / drops the gate for every batch that can take that loop.
 * *gateless: 1 if the last submitted batch ran without the gate; *predicted_pass: the probability the rule used for it (-1: the
 * batch could not take that loop).  Does not synchronise. */
int gs_match_gate_info(gs_run *run, int *gateless, double *predicted_pass);
/* The rule itself, a pure function: would a prefiltered batch of `samples` sampled 15-mers per read on a store of n_lmers distinct
 * canonical 15-mers (-1: never counted) drop the gate?  mode: the value of GS_PF_GATE, -1 when unset.  Returns 1 / 0 and, where
 * predicted_pass is not NULL, the probability 1 - (1 - n_lmers / 2^29)^samples it compares with its bound. */
int gs_match_gate_rule(int64_t n_lmers, int samples, int mode, double *predicted_pass);
/* the device the run's store lives on (for helpers that work beside a run: gs_inflater_create) */
int gs_match_get_device(gs_run *run, int *device);

/* ---------------------------------------------------------------------------------------------------
 * filter
 *
 * Replaces FastqBloomFilter.isAcceptRead (C/bloom/FastqBloomFilter.java:120-161) over a device copy of
 * the reference's index filter: XORKMerBloomFilter / MurmurKMerBloomFilter
 * (C/bloom/AbstractKMerBloomFilter.java:209-216, fields :52-62) or BlockedKMerBloomFilter
 * (C/bloom/BlockedKMerBloomFilter.java:181-199).  The bit array and hash factors are replicated
 * exactly, so false positives are identical.
 *   kind GS_BLOOM_XOR/MURMUR: bits = number of bits, hash_factors[n_hashes]
 *   kind GS_BLOOM_BLOCKED:    bits = number of buckets, hash_factors[0] = seed, n_hashes ignored
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_bloom gs_bloom;
enum { GS_BLOOM_XOR = 0, GS_BLOOM_MURMUR = 1, GS_BLOOM_BLOCKED = 2 };

int gs_bloom_create(gs_bloom **out, int device, int kind, int64_t bits, int32_t n_hashes,
                    const int64_t *hash_factors, const uint64_t *words, int64_t n_words);
/* The index filter built on the device (BloomIndexGoal, C/goals/refseq/BloomIndexGoal.java:66-113): an XORKMerBloomFilter sized
 * for `expected_insertions` k-mers at false-positive rate `fpp` (AbstractKMerBloomFilter.java:172-185: bits, number of hashes;
 * hash factors = the first nextLong() values of java.util.Random(42), :105-109) with putLong of every k-mer (kmers in host or
 * device memory, the reference's encoding -- e.g. the result of gs_dbbuild for the requested taxa).  Bit for bit the filter the
 * reference builds from the same k-mers.  gs_bloom_get returns geometry and contents (words may be NULL; n_words >= (bits+63)/64). */
int gs_bloom_build(gs_bloom **out, int device, int kind, const int64_t *kmers, int64_t n_kmers, int mem, int64_t expected_insertions,
                   double fpp);
int gs_bloom_get(gs_bloom *bloom, int64_t *bits, int32_t *n_hashes, int64_t *hash_factors, uint64_t *words, int64_t n_words);
int gs_bloom_destroy(gs_bloom *bloom);

/* The index goal: BloomIndexGoal.doMakeThis (C/goals/refseq/BloomIndexGoal.java:66-113) on a device store, in one call.
 * requested[n_values] (host): != 0 = the value's node is requested (the per-node flag: any set of values, no subtree implied).
 * The selected k-mers are the store's n_stored pairs (the contract of gs_dbexport_create: reachable, value has a tree node)
 * whose value is requested.  The filter is sized by ensureExpectedSize(count, false) of its kind and filled with putLong of every
 * selected k-mer, bit for bit what the reference builds from the same pairs.  Nothing is exported or sorted on the way.
 *   kind GS_BLOOM_XOR / GS_BLOOM_MURMUR: geometry from (count, fpp), AbstractKMerBloomFilter.java:96-113,172-185;
 *        count == 0 gives bits = 1, n_hashes = 1 (Math.round(+Inf) cast to int is -1, max(1, -1) = 1), no bit set.
 *   kind GS_BLOOM_BLOCKED: BlockedKMerBloomFilter(10 bits per key, seed = Random(42).nextLong()),
 *        buckets = (max(1, count) * 10 + 63) / 64, buckets + 17 words, putLong :109-125; fpp is ignored.
 *   expected_insertions < 0: the count (what the goal does); >= 1: size for this many instead
 *        (hosts that must reproduce a filter sized elsewhere; tests).  0: GS_E_INVALID.
 *   *n_inserted (may be NULL) = the count.
 * Seen bits and `more` bits are masked, so the call may run while a unique-counting run is alive on the store.
 * A partition store (gs_db_create_part) is taken as the part it is.  A stripe of a striped store: GS_E_UNSUPPORTED.
 * More than 64 hashes or more than 2^37 bits: GS_E_UNSUPPORTED, as gs_bloom_build.
 * Every argument is checked before a device is touched. */
int gs_bloom_build_db(gs_bloom **out, gs_db *db, int kind, const uint8_t *requested,
                      int64_t expected_insertions, double fpp, int64_t *n_inserted);

/* What a filter handle knows about itself (gs_bloom_get returns factors and words). */
typedef struct {
    int32_t kind, k;          /* k = 0: unknown (gs_bloom_create, gs_bloom_build)        */
    int32_t n_hashes, pad;
    int64_t bits, n_words;    /* BLOCKED: bits = buckets, n_words = buckets + 17          */
    int64_t expected_insertions, n_inserted;   /* -1: unknown                             */
    double  fpp;              /* 0: unknown                                               */
} gs_bloom_info;
int gs_bloom_get_info(gs_bloom *bloom, gs_bloom_info *info);

/* Native index file, so that a later process filters without rebuilding the index:
 *   header (72 bytes, little endian): magic "GSINDEX1" | int32 kind, k, n_hashes, pad | int64 bits, n_words,
 *       expected_insertions, n_inserted | double fpp | uint64 checksum
 *   hash factors: n_hashes int64 (BLOCKED: n_hashes = 1, the seed)
 *   words: n_words uint64
 * The checksum runs over factors and words (the store file's: over their 32-bit words w, a = 1, b = 0, a += w, b += a,
 * checksum = a ^ (b << 1) ^ (b >> 63), all mod 2^64).  Not portable across versions.  Load checks magic, kind,
 * 1 <= n_hashes <= 64, n_words against bits and kind, the exact file length and the checksum BEFORE a device is touched.
 * A defect: GS_E_INVALID, and the message names the path and the defect.
 * A file that cannot be opened, read or written: GS_E_IO. */
int gs_bloom_save(gs_bloom *bloom, const char *path);
int gs_bloom_load(gs_bloom **out, int device, const char *path);

/* accept[i] = isAcceptRead(read i) ? 1 : 0.  profile != 0 records kernel time (gs_filter_kernel_time). */
int gs_filter_submit(gs_bloom *bloom, int k, int min_pos_count, double positive_ratio, const uint8_t *seq,
                     const uint64_t *offsets, int64_t n_reads, int mem, uint8_t *accept, int profile);
int gs_filter_sync(gs_bloom *bloom);
/* Text mode of the filter, as gs_match_submit_text: a chunk of raw four-line FASTQ, records found (and checked) on the
 * device.  accept[n_lines / 4] as gs_filter_submit; newlines (may be NULL) receives the byte offset of every '\n' of
 * the chunk, i.e. the record geometry the caller needs to rewrite the accepted reads (FastqBloomFilter.java:92-105).
 * Both live in the same memory kind as text and are complete after gs_filter_sync; a refused chunk yields all-zero
 * accept flags and shows up in gs_filter_text_status.  gs_filter_text_reset clears the refusal (and, if asked, the
 * totals of the accepted chunks). */
int gs_filter_submit_text(gs_bloom *bloom, int k, int min_pos_count, double positive_ratio, const uint8_t *text,
                          int64_t n_bytes, int64_t n_lines, int mem, uint8_t *accept, uint32_t *newlines, int profile,
                          int64_t *ticket);
int gs_filter_text_wait_copy(gs_bloom *bloom, int64_t ticket);
int gs_filter_get_device(gs_bloom *bloom, int *device);
int gs_filter_text_status(gs_bloom *bloom, int64_t *failed_ticket, int64_t *first_bad_record, int64_t totals[3]);
int gs_filter_text_reset(gs_bloom *bloom, int clear_totals);

/* FASTA chunks and general (multi-line) FASTQ chunks through the filter: the same record search as gs_match_submit_fasta /
 * gs_match_submit_fastq_ml (AbstractFastqReader.java:375-438, :301-308), the reads gathered on the device, accept[r] per
 * record in file order.  `newlines` (may be NULL) receives the offset of every newline of the chunk (n_lines of them).
 * gs_filter_submit_fastq_ml reports the records that END in the chunk and the bytes / lines they cover (n_records = -1: refused,
 * see gs_filter_text_status; the caller carries the rest into its next chunk).  Afterwards gs_filter_text_read_bounds copies
 * the n_records + 1 offsets of the gathered reads (read lengths = differences) and gs_filter_text_line_classes the class of
 * every line of a general FASTQ chunk (1 descriptor, 2 sequence, 0 '+' / quality); both wait for the chunk. */
int gs_filter_submit_fasta(gs_bloom *bloom, int k, int min_pos_count, double positive_ratio, const uint8_t *text,
                           int64_t n_bytes, int64_t n_lines, int64_t n_records, int mem, uint8_t *accept, uint32_t *newlines,
                           int64_t *ticket);
int gs_filter_submit_fastq_ml(gs_bloom *bloom, int k, int min_pos_count, double positive_ratio, const uint8_t *text,
                              int64_t n_bytes, int64_t n_lines, int mem, uint8_t *accept, uint32_t *newlines,
                              int64_t *n_records, int64_t *consumed_bytes, int64_t *consumed_lines, int64_t *ticket);
int gs_filter_text_read_bounds(gs_bloom *bloom, uint64_t *bounds);
int gs_filter_text_line_classes(gs_bloom *bloom, uint8_t *classes);
int gs_filter_kernel_time(gs_bloom *bloom, int64_t *launches, double *total_ms);

/* ---------------------------------------------------------------------------------------------------
 * Block-gzip input inflated on the device
 *
 * Replaces java.util.zip.GZIPInputStream in front of the FASTQ parser (B/io/StreamProvider.java:92-100, 148-150) for BGZF
 * files (bgzip / htslib; also what this library writes for .gz outputs): gzip members of at most 64 KiB of text that state
 * their compressed size, so the host lists them without inflating and ships the COMPRESSED bytes; one wave inflates one member
 * (genestrip_amd/csrc/gs_inflate_dev.hip), ISIZE and CRC-32 are checked as GZIPInputStream checks them.
 *
 *   payload_offset / payload_len   the member's DEFLATE stream inside `file` (behind the gzip header, in front of the trailer)
 *   isize / crc32                  the member's trailer: size and CRC-32 of its text
 *
 * gs_inflate_members: one shot, host buffers (status[i]: 0 = ok, else the member's inflate error; may be NULL).
 * gs_inflater_*: the streaming form in front of gs_match_submit_text / gs_filter_submit_text.  Every feed appends the text of a
 * run of members behind what the previous feed left over and returns, as DEVICE memory, the longest prefix made of whole
 * four-line records (n_lines a multiple of 4, n_bytes up to and including that newline); the rest is carried into the next
 * feed.  next_lo / next_hi: the byte range of `file` the NEXT feed will need (0, 0: none) -- it is copied to the device while
 * this feed's kernels run.  The returned pointer stays valid until the NEXT feed (hand it to gs_match_submit_text with
 * GS_MEM_DEVICE and wait for that chunk's copy -- gs_match_text_wait_copy -- before feeding again).  gs_inflater_tail: what is left after the last feed (fewer
 * than four lines, or a last line without newline), for the caller's parser.  A member that does not inflate to its ISIZE and
 * CRC-32 fails the feed with GS_E_INVALID (gs_inflate_last_error).
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t payload_offset;
    uint32_t payload_len;
    uint32_t isize;
    uint32_t crc32;
    uint32_t reserved;
} gs_inflate_member;
typedef struct gs_inflater gs_inflater;
int gs_inflate_members(int device, const uint8_t *file, const gs_inflate_member *members, int64_t n_members, uint8_t *out,
                       int64_t out_cap, int32_t *status);
int gs_inflater_create(gs_inflater **out, int device);
int gs_inflater_feed(gs_inflater *inf, const uint8_t *file, const gs_inflate_member *members, int64_t n_members, int64_t next_lo,
                     int64_t next_hi, int last, const uint8_t **text, int64_t *n_bytes, int64_t *n_lines, int64_t *tail_bytes);
/* A SINGLE-MEMBER gzip stream (gzip, pigz) inflated on the device: block boundaries found speculatively, segments decoded side by
 * side with markers for the unknown 32 KiB window, windows resolved in a second pass (gs_inflate_dev.hip), CRC-32 and ISIZE checked
 * as java.util.zip.GZIPInputStream does (B/io/StreamProvider.java:92-100).
 * gs_gunzipper_*: the stream in BATCHES of about one segment per wave slot of the device (a file of any size through buffers of a few
 * gigabytes).  gs_gunzipper_next: the text of the next batch in device memory, behind the last `keep_tail` bytes of the text the call
 * before returned (what lay behind the caller's last whole record); the pointer is valid until the next call.  *last: 0 = more
 * batches follow, 1 = the file is through (every member's CRC-32 and ISIZE were right; members behind one another -- cat a.gz b.gz --
 * give their texts behind one another, what is not a member behind the last trailer is ignored as GZIPInputStream ignores it).
 * GS_E_UNSUPPORTED (from open or from any batch): not a stream this
 * path takes from here on (a segment that outgrows its buffer, a block boundary that was a mirage and could not be repaired) -- the
 * caller inflates the rest on the host; GS_E_INVALID: the stream is damaged (bad code, CRC-32 or ISIZE mismatch).  `gz` must stay
 * readable until gs_gunzipper_close, _reopen or _park (a stream of up to 16 GiB is uploaded by a thread of the object's own while the
 * batches are decoded).  gs_gunzipper_info: [0] segments, [1] chunks searched, [2] batches, [3] block starts that were
 * mirages (decoded again).
 * gs_gunzip_plan_device: the whole stream into ONE device buffer (released with gs_gunzip_free; several members: GS_E_UNSUPPORTED);
 * gs_gunzip_device copies it to `out` (tests, tools).  info as gs_gunzipper_info. */
typedef struct gs_gunzipper gs_gunzipper;
int gs_gunzipper_open(gs_gunzipper **out, int device, const uint8_t *gz, int64_t n);
int gs_gunzipper_reopen(gs_gunzipper *g, const uint8_t *gz, int64_t n); /* the same object and its device buffers on another file */
int gs_gunzipper_next(gs_gunzipper *g, int64_t keep_tail, const uint8_t **d_text, int64_t *n_text, int *last);
int gs_gunzipper_info(const gs_gunzipper *g, int64_t info[4]);
int gs_gunzipper_first_span(gs_gunzipper *g, int64_t bytes); /* the first batch takes at most `bytes` of compressed data: first text early (callers with writers) */
int gs_gunzipper_park(gs_gunzipper *g); /* the caller is through with the file: the upload thread is stopped (`gz` may go away), the buffers stay */
int gs_gunzipper_close(gs_gunzipper *g);
int gs_gunzip_plan_device(int device, const uint8_t *gz, int64_t n, uint8_t **d_text, int64_t *n_text, int64_t info[4]);
int gs_gunzip_free(int device, uint8_t *d_text);
int gs_gunzip_device(int device, const uint8_t *gz, int64_t n, uint8_t *out, int64_t out_cap, int64_t *n_text, int64_t info[4]);
/* lines and the offset behind the last newline that closes a four-line record (count a multiple of four) in n bytes of device text */
int gs_text_cut_device(int device, const uint8_t *d_text, int64_t n, int64_t *n_lines, int64_t *cut);
/* n bytes of device memory to host memory (page-locked for speed); synchronous */
int gs_device_fetch(int device, const uint8_t *d_src, uint8_t *out, int64_t n);
int gs_inflater_tail(gs_inflater *inf, uint8_t *out, int64_t cap, int64_t *n);
/* the first n_bytes of the text the LAST gs_inflater_feed returned, copied to host memory (page-locked for speed); synchronous.
 * For callers that need the text on the host as well -- the filter goal's writers (C/bloom/FastqBloomFilter.java:92-105 rewriteInput). */
int gs_inflater_fetch(gs_inflater *inf, uint8_t *out, int64_t n_bytes);
int gs_inflater_reset(gs_inflater *inf);  /* ready for another file; its device and page-locked buffers stay (allocating them costs more than inflating a file) */
int gs_inflater_destroy(gs_inflater *inf);
const char *gs_inflate_last_error(void);

/* ---------------------------------------------------------------------------------------------------
 * The output side on the device (genestrip_amd/csrc/gs_deflate_dev.hip)
 *
 * Replaces, for the records of a four-line text chunk, the per-read writers of the reference: ReadEntry.write
 * (C/fastq/AbstractFastqReader.java:570-584) as called by FastqBloomFilter.nextEntry -> rewriteInput (C/bloom/FastqBloomFilter.java:92-105,
 * AbstractFastqReader.java:465-470) and by FastqKMerMatcher.afterMatch (C/match/FastqKMerMatcher.java:304-307), and the
 * java.util.zip.GZIPOutputStream behind them (B/io/StreamProvider.java getOutputStreamForFile; gzipFastqOutput is the reference's
 * default, C/GSConfigKey.java:155).
 *
 * gs_filter_compact_text / gs_match_compact_text: the records of the handle's most recent four-line chunk (gs_filter_submit_text /
 * gs_match_submit_text with per-read flags; it must not have been refused) that the writer wants -- filter: accept flag set
 * (which != 0) or clear (which == 0: the reference's dump file); match: GS_F_RETURNED set -- rewritten exactly as ReadEntry.write
 * does (descriptor, '\n', read, "\n+\n", the record's quality line if with_probs else '~' x length, '\n'), back to back in a
 * device buffer of the handle's: *d_out (valid until the next compact call with the same `which` and `slot`; slot 0 / 1: two
 * buffers, so that chunk i can be on its way out while chunk i + 1 is gathered), *n_bytes, *n_records.  To be called before the
 * next chunk is submitted on the handle.  Synchronises the handle's stream.
 *
 * gs_deflater_*: n bytes of device text -> block-gzip (BGZF) members in host memory: gzip members (RFC 1952) of at most 63 KiB of
 * text, each with its size in a 'BC' extra subfield (what bgzip writes; GZIPInputStream / zcat read the file as one stream, this
 * library's device inflater takes the members side by side).  One wave per member: run / hash matches chosen per lane, greedy
 * parse, Huffman code from a counting pass over a sample of the call's text, built on the host, shared by the call's members;
 * CRC-32 and ISIZE as GZIPOutputStream writes them.  out_cap >= gs_deflate_bound(n).  No end-of-file block (28 bytes, the
 * caller's: an empty member).  Synchronous.  gs_deflate_host: host text through the same path (tests, tools);
 * gs_deflate_host_reference: the same format from a plain CPU loop over the same tables (a test of the table builder that runs
 * without a device).  gs_deflater_info: [0] members, [1] text bytes, [2] compressed bytes so far.
 * gs_deflater_append / _pending / _flush: chunks of a few MiB are better compressed together (a call costs ~0.6 ms whatever its
 * size): append copies d_text[0, n) behind the text that is waiting on the device (the source is free when it returns), flush
 * compresses what waits (out_cap >= gs_deflate_bound(gs_deflater_pending(d))).
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_deflater gs_deflater;
int gs_filter_compact_text(gs_bloom *bloom, int which, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records);
int gs_match_compact_text(gs_run *run, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records);
/* The same for the handle's most recent FASTA or general FASTQ chunk (gs_*_submit_fasta / _fastq_ml, gs_reads_select_fasta /
 * _fastq_ml), by the kernels of gs_rewrite.hip: the descriptor line (FASTA: its first byte replaced by '@'), '\n', the read in ONE
 * line ('\r's of its lines kept), "\n+\n", then '~' x length or -- with_probs on a general FASTQ chunk -- every line of the record
 * behind its '+' line, joined (at least as many bytes as the read), '\n'.  Only the records that END in a general FASTQ chunk count.
 * Which records: filter: as `which` says; match: GS_F_RETURNED set; reads: selected.  *d_out: a buffer of the handle's, valid until
 * the next call with the same slot (0 / 1) and, for the filter, the same `which`.  Synchronises the handle's stream; to be called before the next submit.  A chunk of
 * zero records: GS_OK and 0 bytes.  GS_E_STATE: no chunk submitted, the last one was four-line FASTQ, was refused or was submitted
 * without per-read flags. */
int gs_filter_compact_records(gs_bloom *bloom, int which, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records);
int gs_match_compact_records(gs_run *run, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records);

/* ---- Kraken-style lines of a four-line chunk as device text (gs_kraken.hip) -------------------------------------------------
 * taxid string per value index (SmallTaxIdNode.getTaxId), copied to the run's device: bytes back to back + n_values + 1 offsets.
 * NULL entries: GS_E_INVALID.  Any bytes, any length (0 included).  May be called again; replaces the earlier set. */
int gs_match_set_taxids(gs_run *run, const char *const *taxids);
/* The Kraken-style lines (FastqKMerMatcher.java:308-314, :597-611, :723-756) of the most recent FOUR-LINE text chunk of the run,
 * in read order, as device text.  *d_out: a buffer of the run's, valid until the next call with the same slot (0 / 1);
 * *n_bytes, *n_lines: what was written.  Synchronises the run's stream, as gs_match_compact_text does.
 * To be called before the next submit on the run.  GS_E_STATE: no chunk submitted, the last one was FASTA or general FASTQ, was
 * refused, was submitted without a class array, or no taxids are set.  Afterwards gs_match_segments_fetch returns this chunk's
 * segments (the call computes them as gs_match_segments_text does). */
int gs_match_kraken_text(gs_run *run, int write_all, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_lines);
/* The same for the most recent FASTA or general FASTQ chunk of the run: the name comes from the record's descriptor line (behind its
 * first byte, '>' or '@' alike, up to the first blank), the length is that of the gathered read; a record without a k-mer position
 * (a FASTA header without sequence lines) has no line.  GS_E_STATE: no chunk submitted, the last one was four-line FASTQ, was
 * refused, was submitted without a class array, or no taxids are set.  Shares the slots and buffers of gs_match_kraken_text. */
int gs_match_kraken_records(gs_run *run, int write_all, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_lines);
/* accumulated device time of the text kernels of gs_match_kraken_text / _records since gs_match_begin (cfg.profile != 0): one event pair
 * around the size pass (sizes, prefix, offsets) and one around the write pass of every call -- `launches` counts the pairs; neither
 * the segments nor the read-back of the text's size between the two passes is in it */
int gs_match_kraken_time(gs_run *run, int64_t *launches, double *total_ms);
int gs_deflater_create(gs_deflater **out, int device);
int gs_deflater_pack(gs_deflater *d, const uint8_t *d_text, int64_t n, uint8_t *out, int64_t out_cap, int64_t *n_out);
int gs_deflater_info(const gs_deflater *d, int64_t info[3]);
int gs_deflater_append(gs_deflater *d, const uint8_t *d_text, int64_t n);
int64_t gs_deflater_pending(const gs_deflater *d);
int gs_deflater_flush(gs_deflater *d, uint8_t *out, int64_t out_cap, int64_t *n_out);
int gs_deflater_destroy(gs_deflater *d);
int64_t gs_deflate_bound(int64_t n);
int gs_deflate_host(int device, const uint8_t *text, int64_t n, uint8_t *out, int64_t out_cap, int64_t *n_out);
int gs_deflate_host_reference(const uint8_t *text, int64_t n, uint8_t *out, int64_t out_cap, int64_t *n_out);
const char *gs_deflate_last_error(void);

/* ---------------------------------------------------------------------------------------------------
 * Read streams without a store or a filter (genestrip_amd/csrc/gs_rewrite.hip): the extract goal (C/goals/ExtractGoal.java:73-129)
 * and the fasta2fastq goal (C/goals/Fasta2FastqGoal.java:92-165).  A gs_reads handle owns the same text stage as a run or a filter:
 * its own stream, staging, status words and totals; chunk contracts, refusal rules and status reporting of the three select calls
 * are those of gs_filter_submit_text / _fasta / _fastq_ml (k only feeds the totals).
 *
 * gs_reads_select_*: accept[r] = 1 iff the descriptor line of record r behind its first byte -- up to but excluding the '\n', a
 * '\r' included -- holds at least key_len bytes and starts with the key (ByteArrayUtil.startsWith(readDescriptor, 1, key),
 * ExtractGoal.java:93); FASTA records use their header line the same way.  key_len < 1, a NUL byte or a byte >= 0x80 in the key:
 * GS_E_INVALID (the goal does nothing for an empty key; Java compares byte != char, such a byte never matches).
 * gs_reads_compact_text: the selected records of the most recent chunk as ReadEntry.write writes them (as gs_filter_compact_text
 * with which = 1): of a four-line chunk by the gather of gs_deflate_dev.hip, of a FASTA chunk by the FASTA -> FASTQ kernel in its
 * ReadEntry mode ('@' header[1:] '\n' sequence "\n+\n" '~' x L '\n', the sequence = the data lines without their '\n', '\r'
 * kept; with_probs changes nothing: FASTA has no qualities).  General FASTQ chunks: GS_E_UNSUPPORTED (the host's writers).
 * gs_reads_fasta2fastq: the FASTQ text of ALL records of a FASTA chunk of whole records as the fasta2fastq goal prints them:
 * the header from byte 1 up to the '\n' ('\r' stays), every data line without its trailing '\r's and '\n' (empty lines are data
 * lines of zero bytes), '~' x the bytes kept; a record without data gives "@h\n\n+\n\n".  The chunk starts with '>', ends with
 * '\n', n_lines / n_records are its newlines and header lines; mem: GS_MEM_HOST or GS_MEM_DEVICE.  Refused (gs_reads_text_status;
 * *d_out = NULL, *n_bytes_out = 0) are only chunks that do not start with '>', hold a NUL byte (the reference's line reader
 * drops those) or whose counts are wrong.  *long_lines (may be NULL) = lines of 65 534 bytes or more incl. the newline: the
 * reference throws there (AbstractFastaReader.java:104-106), the text is made all the same.  Bytes >= 0x80 are copied as they
 * are (the reference's PrintStream widens them: the host layer's case).  *d_out: a device buffer of the handle's, valid until
 * the next call with the same slot (0 / 1).  Synchronises the handle's stream, as gs_reads_compact_text does.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_reads gs_reads;
int gs_reads_create(gs_reads **out, int device);
int gs_reads_destroy(gs_reads *reads);
int gs_reads_get_device(gs_reads *reads, int *device);
int gs_reads_sync(gs_reads *reads);
/* profile != 0: from now on the FASTA -> FASTQ text kernels (sizes, offsets, copy) of gs_reads_compact_text and gs_reads_fasta2fastq
 * run between events; launches / total_ms (may be NULL) = what they add up to so far.  Synchronises. */
int gs_reads_kernel_time(gs_reads *reads, int profile, int64_t *launches, double *total_ms);
/* What a profiling handle has measured so far, phase by phase, as time on its stream between events: [0] the select calls, from a
 * chunk's submission to its flags (its way in, the record search, the descriptor compare); [1] the four-line gather of
 * gs_reads_compact_text; [2] the FASTA -> FASTQ text kernels (as gs_reads_kernel_time).  Synchronises. */
int gs_reads_phase_times(gs_reads *reads, int64_t launches[3], double total_ms[3]);
int gs_reads_select_text(gs_reads *reads, int k, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, const uint8_t *key,
                         int32_t key_len, uint8_t *accept, uint32_t *newlines, int64_t *ticket);
int gs_reads_select_fasta(gs_reads *reads, int k, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int64_t n_records, int mem,
                          const uint8_t *key, int32_t key_len, uint8_t *accept, uint32_t *newlines, int64_t *ticket);
int gs_reads_select_fastq_ml(gs_reads *reads, int k, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, const uint8_t *key,
                             int32_t key_len, uint8_t *accept, uint32_t *newlines, int64_t *n_records, int64_t *consumed_bytes,
                             int64_t *consumed_lines, int64_t *ticket);
int gs_reads_compact_text(gs_reads *reads, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records);
/* the selected records of the most recent FASTA or general FASTQ chunk, the latter with its quality lines where with_probs asks for
 * them: see gs_filter_compact_records.  Its launches count in gs_reads_kernel_time and in [2] of gs_reads_phase_times. */
int gs_reads_compact_records(gs_reads *reads, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records);
int gs_reads_fasta2fastq(gs_reads *reads, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int64_t n_records, int mem, int slot,
                         const uint8_t **d_out, int64_t *n_bytes_out, int64_t *long_lines, int64_t *ticket);
int gs_reads_text_read_bounds(gs_reads *reads, uint64_t *bounds);
int gs_reads_text_line_classes(gs_reads *reads, uint8_t *classes);
int gs_reads_text_wait_copy(gs_reads *reads, int64_t ticket);
int gs_reads_text_status(gs_reads *reads, int64_t *failed_ticket, int64_t *first_bad_record, int64_t totals[3]);
int gs_reads_text_reset(gs_reads *reads, int clear_totals);

/* ---------------------------------------------------------------------------------------------------
 * Measurement support (no reference counterpart; not on the data path): the ceilings of the device the kernels run on,
 * measured with small calibration kernels at the match kernel's occupancy (8 waves per SIMD), so that a benchmark prices
 * its kernels against numbers taken in the same process on the same chip (bench.py `roofline`).
 *   out[0] = rate: wave64 instructions per second over the whole device (VALU_PURE: full-rate 32-bit ops; VALU_MIX: the
 *            match kernel's instruction mix; SALU; VALU_SALU: an alternating stream, both kinds counted), wave-level load
 *            instructions per second (VMEM_*: byte loads of 64 consecutive bytes / dword loads of 8 distinct words /
 *            16-byte loads with 8 lanes per 64-byte line / 16-byte loads with a line per lane, all cache resident), or
 *            random 64-byte lines per second from a table of `arg` bytes (RANDOM_LINES)
 *   out[1] = milliseconds of the timed launch, out[2] = instructions / loads / lines it issued, out[3] = compute units */
enum {
    GS_CAL_VALU_PURE = 0, GS_CAL_VALU_MIX = 1, GS_CAL_SALU = 2, GS_CAL_VALU_SALU = 3,
    GS_CAL_VMEM_BYTES = 4, GS_CAL_VMEM_WORDS = 5, GS_CAL_VMEM_SHARED_LINES = 6, GS_CAL_VMEM_SCATTERED = 7,
    GS_CAL_RANDOM_LINES = 8
};
int gs_calibrate(int device, int what, int64_t arg, double out[4]);

/* ---------------------------------------------------------------------------------------------------
 * krakencount: Kraken-style output lines counted per tax id (genestrip_amd/csrc/gs_krakencount.hip)
 *
 * Replaces KrakenResultProcessor.process (C/kraken/KrakenResultProcessor.java:74-179) under the listener of KrakenResCountGoal
 * (C/goals/kraken/KrakenResCountGoal.java:133-157) for chunks of whole lines inside the grammar stated at the head of
 * gs_krakencount.hip.  A chunk outside it -- or one whose new tax ids the table cannot take -- is REFUSED: it adds nothing, the
 * caller counts it with the reference-exact parser (include/gshost.h).  A refusal is not sticky: the next chunk is taken on its
 * own merits.  An empty line is no refusal: the lines in front of it count, the chunk reports its byte offset (the reference stops
 * reading there).  Deliberate difference: a line of more than 65 536 bytes with its newline makes the reference fail (array
 * index); here it counts like any other and is reported in the long-lines total.
 *
 * A handle owns its stream, its staging and its table of up to max_taxids rows (open addressing over the tax id as uint32).
 * gs_krakencount_geometry: [0] bytes per tile (one workgroup, one flush of its LDS table), [1] slots of that LDS table, [2] slots
 * of the global table, [3] the highest level of the prefix sums in use (1: inside a scan block, 2: one thread per block sum,
 * 3: a run of block sums per thread), [4] bytes per scan block, [5] scan blocks from which level 3 is in play.
 * gs_krakencount_submit: text = n_bytes (at most 1 GiB) of whole lines, the last byte a newline; mem: GS_MEM_HOST (free again on
 * return) or GS_MEM_DEVICE (free again after the next synchronising call).  *ticket: 0, 1, ... in submission order.
 * gs_krakencount_chunk: what became of one of the last 64 chunks: [0] 0 counted / 1 outside the grammar / 2 table full, [1] its
 * first bad line (0-based, -1: none), [2] the offset of its first empty line (-1), [3] rows of the table behind it, [4..7] its
 * lines, counted tokens, skipped 'A' tokens, long lines.  Synchronises, as do _status, _fetch, _counters and _kernel_time.
 * gs_krakencount_status: the first refused chunk since the last reset (-1: none) and its first bad line (-1 for a full table),
 * the first-empty-line offset of the most recent chunk, totals = lines, counted tokens, skipped 'A' tokens, long lines.
 * gs_krakencount_fetch: *n_rows rows (all of them are written if cap >= *n_rows, else none) in the order of DigitTrie.collect
 * (C/util/DigitTrie.java:294-305) over the decimal strings; counts[3 * i ..] = reads, kmers, kmers in matching reads.
 * gs_krakencount_counters: [0] global atomics issued by the accumulation, [1] tokens whose key found no room in a workgroup's table.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_krakencount gs_krakencount;
int gs_krakencount_create(gs_krakencount **out, int device, int64_t max_taxids);
int gs_krakencount_destroy(gs_krakencount *kc);
int gs_krakencount_get_device(gs_krakencount *kc, int *device);
int gs_krakencount_geometry(gs_krakencount *kc, int64_t geometry[6]);
int gs_krakencount_submit(gs_krakencount *kc, const uint8_t *text, int64_t n_bytes, int mem, int64_t *ticket);
int gs_krakencount_chunk(gs_krakencount *kc, int64_t ticket, int64_t report[8]);
int gs_krakencount_status(gs_krakencount *kc, int64_t *failed_ticket, int64_t *first_bad_line, int64_t *first_empty_offset, int64_t totals[4]);
int gs_krakencount_reset(gs_krakencount *kc);
int gs_krakencount_fetch(gs_krakencount *kc, int32_t *taxids, int64_t *counts, int64_t cap, int64_t *n_rows);
int gs_krakencount_counters(gs_krakencount *kc, int64_t counters[2]);
/* profile != 0: from now on the kernels of every chunk run between events; launches / total_ms: what they add up to so far */
int gs_krakencount_kernel_time(gs_krakencount *kc, int profile, int64_t *launches, double *total_ms);

/* ---------------------------------------------------------------------------------------------------
 * genomes: genome FASTA text to the regions of a build (genestrip_amd/csrc/gs_genomes.hip)
 *
 * Replaces the line walk of AbstractFastaReader.readFasta (C/fasta/AbstractFastaReader.java:97-130) over
 * BufferedLineReader.nextLine (B/io/BufferedLineReader.java:160-182) and the strip of AbstractStoreFastaReader.dataLine
 * (C/refseq/AbstractStoreFastaReader.java:87-114) in front of gs_dbsize_add / gs_dbbuild_add / gs_dbupdate_add / gs_dbquality_add.
 * The device does the text work only: which records count, and for which node, is the caller's decision (accession map, tree,
 * limits), taken from the header lines the scan hands out and given back as one flag per record.
 *
 * A record is a header line (first byte '>') and the data lines up to the next header line.  Of a data line the trailing run of
 * '\n' / '\r' is stripped, every other byte is a base of the region ('\r' with a byte of its line behind its run, lower case and
 * '>' inside a line included); empty lines give nothing; a header line without data lines is a region of 0 bases; data lines in
 * front of the first header line of the text belong to no region.  The last line may lack its newline.
 *
 * gs_genomes_scan     text: n_bytes (at most 1 GiB, more: GS_E_UNSUPPORTED) in host or device memory (mem), free again on return
 *                     (the handle works on a copy).  last != 0: the stream ends with this chunk.  *n_records: the records that
 *                     END inside the chunk -- those in front of its last header line, with `last` all of them; *consumed_bytes:
 *                     the bytes they cover (the offset of that last header line; without any header line: behind the last
 *                     newline; with `last`: n_bytes).  The caller puts text[*consumed_bytes ..] in front of the next chunk; if
 *                     nothing was consumed it grows the chunk, and a record that does not fit 1 GiB is the host parser's.
 *                     *header_bytes: bytes of the records' header lines ('>' up to but excluding the '\n', a '\r' included).
 *                     *max_line_bytes: the longest line in front of the cut with its newline (the reference throws when a line
 *                     reaches fastaLineSizeBytes - 1; here that is the caller's to report).
 *                     REFUSED with GS_E_UNSUPPORTED -- the message names the first bad byte offset -- is a chunk with a NUL byte
 *                     (the reference drops it before it looks at the line) or with a run of more than 64 '\r' (the look-ahead of
 *                     the strip rule is bounded): such a chunk belongs to the host parser (include/gshost.h); the handle stays
 *                     usable and holds no chunk.
 *                     A chunk of 2^24 header lines or more is GS_E_UNSUPPORTED as well (the message gives the count; the
 *                     selection keeps the kept records in 24 bits): the caller cuts it; nothing was consumed.
 * gs_genomes_headers  the header lines back to back and header_off[n_records + 1] (host arrays, header_bytes / n_records + 1).
 * gs_genomes_gather   keep[n_records] (host; != 0: kept; NULL: every record) -> the bases of the kept records alone, in order, as
 *                     seq / off[*n_regions + 1] (uint64 from 0) on the device.  May be called again with other flags.
 * gs_genomes_regions  the device arrays of the last gather, in the form every _add call takes with GS_MEM_DEVICE.  Valid until the
 *                     next scan, gather or destroy on this handle.  They are complete when gather returns (it synchronises),
 *                     and all four _add calls synchronise their own stream before they return, so an _add that has returned
 *                     no longer reads them: no fence is needed between _add and the next scan.
 * gs_genomes_kernel_time  time between events on the handle's stream so far: the scan kernels, the select and gather kernels.
 * Call order: scan, then headers / gather in any order and number, regions behind a gather; anything else: GS_E_STATE, as after a
 * refused scan.  NULL or negative arguments: GS_E_INVALID, before any device call.  Device buffers grow by doubling.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_genomes gs_genomes;
int gs_genomes_create(gs_genomes **out, int device);
int gs_genomes_scan(gs_genomes *g, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t *n_records, int64_t *consumed_bytes,
                    int64_t *header_bytes, int64_t *max_line_bytes);
int gs_genomes_headers(gs_genomes *g, uint8_t *headers, uint64_t *header_off);
int gs_genomes_gather(gs_genomes *g, const uint8_t *keep, int64_t *n_regions, int64_t *n_bases);
int gs_genomes_regions(gs_genomes *g, const uint8_t **d_seq, const uint64_t **d_off);
int gs_genomes_kernel_time(gs_genomes *g, double *ms_scan, double *ms_gather);
int gs_genomes_destroy(gs_genomes *g);

/* ---------------------------------------------------------------------------------------------------
 * accmap: lines of a RefSeq catalog to the accession map (genestrip_amd/csrc/gs_accmap.hip)
 *
 * Replaces AccessionFileProcessor.processCatalog (C/refseq/AccessionFileProcessor.java:96-131) under AccessionMapSizeGoal
 * (C/goals/refseq/AccessionMapSizeGoal.java:70-103: the count of passing entries) and AccessionMapGoal
 * (C/goals/refseq/AccessionMapGoal.java:82-114: the put of every passing entry whose tax id names a node), the sort of
 * AccessionMapImpl.optimize (C/refseq/AccessionMapImpl.java:123-145) and the search of AccessionMapImpl.get (:59-74) under
 * AbstractRefSeqFastaReader.updateNodeFromInfoLine (C/refseq/AbstractRefSeqFastaReader.java:228-239), for chunks of whole lines
 * inside the grammar stated at the head of gs_accmap.hip.  A chunk outside it is REFUSED: it leaves the handle as it was, and the
 * caller parses it line by line (genestrip_amd/csrc/gs_accmapparse.h) and hands its entries in through gs_accmap_append, so that
 * the input order -- which decides among equal keys -- is kept.
 *
 * The tree reaches the handle as known_taxids[n_nodes]: ascending, distinct, positive.  A node is its index in that array; -1 is
 * "none".  A key is a 32-byte slot: byte 0 the length of the accession (0..31), bytes 1..31 the accession, zero-padded.  Read as
 * four big-endian 64-bit words, slots order as AccessionMapImpl.compareBytes orders keys (length, then bytes: all are below 0x80).
 * The reference keeps equal keys and which of them a search finds depends on its quicksort; here gs_accmap_lookup answers with
 * the entry that came FIRST in the input -- a deliberate choice.
 *
 * gs_accmap_create   cfg: the three prefix flags (SeqType GENOMIC: dna; RNA: rna; M_RNA: mrna; ALL_RNA: rna + mrna; ALL: all
 *                    three), category and status strings (searched for as substrings of the fourth and fifth field; 1..32 bytes
 *                    each, at most 16 of each kind, at least one of each), the tree, entries to make room for at once.
 *                    device -1: a HOST-ONLY map, for callers without a device (include/gshost.h under GS_HOST_FAST=0): it touches
 *                    no device, takes entries through gs_accmap_append alone (gs_accmap_submit and gs_accmap_lookup_genomes:
 *                    GS_E_UNSUPPORTED), sorts and searches on the host and answers gs_accmap_lookup for host memory.
 * gs_accmap_submit   text: n_bytes (at most 1 GiB) of whole lines in host or device memory (mem), free again on return.  last != 0:
 *                    the stream ends here and its final line need not be terminated.  report: [0] lines, [1] passing entries (the
 *                    accmapsize count), [2] entries put, [3] 1: refused (then [1] and [2] are 0 and the caller owes them),
 *                    [4] the first bad line (0-based; -1: none), [5] the longest line with its newline, [6] [7] 0.
 * gs_accmap_append   n entries made elsewhere: keys32 (n slots), nodes (n indices into known_taxids), host memory; n_passing: the
 *                    passing entries of the same lines (those without a node included), added to the size count.
 * gs_accmap_finish   sorts; info: [0] entries, [1] passing entries in all, [2] entries equal to the one in front of them,
 *                    [3] those of them with another node.  Behind it submit and append are GS_E_STATE; in front of it fetch and
 *                    the lookups are.
 * gs_accmap_fetch    host arrays, any of them NULL: the sorted slots (32 * entries bytes), their nodes, regions[n_nodes] (entries per
 *                    node: TaxIdNode.incRefSeqRegions).
 * gs_accmap_lookup   n header lines headers[header_off[i] .. header_off[i + 1]) ('>' first; newline or not), mem: where headers,
 *                    header_off and node_out live.  node_out[i]: the node of the accession [1, first blank), -1 if the line has no
 *                    blank, if complete_only != 0 and the accession starts with none of AC_ NC_ NZ_ NM_ XM_ NR_ XR_, or if the
 *                    map does not hold it.
 * gs_accmap_lookup_genomes  the same over the header lines of the chunk that g has scanned (gs_genomes_scan; same device), which
 *                    never leave the device; node_out: host, one per record.
 * gs_accmap_get_n_nodes  the n_nodes of the cfg the map was created with: what a table per node must have.
 * gs_accmap_kernel_time  profile != 0: from now on scan, finish and lookup run between events; what they add up to so far.
 * NULL or negative arguments: GS_E_INVALID, before any device call.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_accmap gs_accmap;
typedef struct {
    int32_t dna, rna, mrna;
    int32_t n_categories, n_statuses;
    int32_t n_nodes;
    const char *const *categories;
    const char *const *statuses;
    const int32_t *known_taxids;
    int64_t reserve_entries;
} gs_accmap_cfg;
int gs_accmap_create(gs_accmap **out, int device, const gs_accmap_cfg *cfg);
int gs_accmap_submit(gs_accmap *am, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t report[8]);
int gs_accmap_append(gs_accmap *am, const uint8_t *keys32, const int32_t *nodes, int64_t n, int64_t n_passing);
int gs_accmap_finish(gs_accmap *am, int64_t info[4]);
int gs_accmap_fetch(gs_accmap *am, uint8_t *keys32, int32_t *nodes, int32_t *regions);
int gs_accmap_lookup(gs_accmap *am, const uint8_t *headers, const uint64_t *header_off, int64_t n, int mem, int complete_only, int32_t *node_out);
int gs_accmap_lookup_genomes(gs_accmap *am, gs_genomes *g, int complete_only, int32_t *node_out);
int gs_accmap_get_device(gs_accmap *am, int *device);
int gs_accmap_get_n_nodes(gs_accmap *am, int32_t *n_nodes);
int gs_accmap_kernel_time(gs_accmap *am, int profile, int64_t *launches, double *total_ms);
int gs_accmap_destroy(gs_accmap *am);

/* ---------------------------------------------------------------------------------------------------
 * asmsum: lines of a Genbank assembly summary to the picks per tree node (genestrip_amd/csrc/gs_asmsum.hip)
 *
 * Replaces AssemblySummaryReader.getRelevantEntries (C/genbank/AssemblySummaryReader.java:104-144) and the cap of
 * FastaFilesFromGenbankGoal (C/goals/genbank/FastaFilesFromGenbankGoal.java:101-150), the fastasgenbank goal, for chunks of whole
 * lines inside the grammar stated at the head of gs_asmsum.hip: no CR, no line above 4096 bytes with its newline, no byte from 0x80
 * on in the key field of a record of 20 fields and more, no kept entry with an empty ftp field.  A chunk outside it is REFUSED: it
 * leaves the handle as it was, and the caller parses it record by record (genestrip_amd/csrc/gs_asmsumparse.h) and hands its
 * entries in through gs_asmsum_append, so that the input order -- which decides at the cut of the cap -- is kept.
 *
 * The tree reaches the handle as known_taxids[n_nodes]: ascending, distinct, positive, at most 9 digits.  A node is its index in that
 * array.  A quality is the ordinal of AssemblyQuality: 1 COMPLETE_LATEST, 2 COMPLETE, 3 CHROMOSOME_LATEST, 4 CHROMOSOME,
 * 5 SCAFFOLD_LATEST, 6 SCAFFOLD, 7 CONTIG_LATEST, 8 CONTIG, 9 LATEST, 10 NONE.  A line is 0-based and counts every line of the stream,
 * comment and empty ones too.  The reference's result is a HashMap; here the nodes come out in ascending order, and the tax id,
 * species tax id and ftp path of an entry are the file's bytes, not decoded strings.
 *
 * gs_asmsum_create   cfg: the tree; filter: n_nodes flags (the taxfromgenbank set) or NULL for every node; quality_mask: bit q allows
 *                    ordinal q, -1 is the reference's null list (all), 0 allows none; reference_only; use_species_taxid: the key is
 *                    field 6, not field 5; entries to make room for at once.  device -1: a HOST-ONLY handle: it touches no device,
 *                    takes entries through gs_asmsum_append alone (gs_asmsum_submit: GS_E_UNSUPPORTED), and finishes and fetches
 *                    on the host.
 * gs_asmsum_submit   text: n_bytes (at most 1 GiB) of whole lines in host or device memory (mem), free again on return.  last != 0:
 *                    the stream ends here and its final line need not be terminated.  report: [0] counted records (20 fields and
 *                    more), [1] kept entries, [2] records of fewer than 20 fields, [3] 1: refused (then [0] [1] [2] are 0 and the
 *                    caller owes them), [4] the first line outside the grammar (0-based in the chunk; -1: none), [5] the longest
 *                    line with its newline, [6] comment and empty lines, [7] bytes added to the string pool.
 * gs_asmsum_append   n entries made elsewhere, host memory, in input order: nodes, quality, is_ref, lines (of the whole stream),
 *                    str_off[3 n + 1] into pool (tax id, species tax id, ftp path of each; the ftp path is not empty).  n_counted:
 *                    the counted records of the same lines; n_lines: those lines, all of them: the next submit's first line
 *                    follows them.
 * gs_asmsum_finish   the cap: per node, if max_per_node > 0 and the node has more entries, they are sorted stably, highest ordinal
 *                    first, and cut from the front until max_per_node remain; a node that is not cut keeps input order.  info:
 *                    [0] kept entries, [1] picked entries, [2] nodes with entries, [3] counted records in all.  Behind it submit
 *                    and append are GS_E_STATE; in front of it fetch is.
 * gs_asmsum_fetch    host arrays, any of them NULL: the picked entries grouped by ascending node, inside a node in the reference's
 *                    list order: nodes, quality, is_ref, lines (info[1] each), str_off[3 * info[1] + 1] into pool.
 * gs_asmsum_file_name  AssemblyEntry's file name of an ftp path of n >= 1 bytes: the bytes behind its last '/', or, if that is its
 *                    last byte, between the '/' in front of it and it, and "_genomic.fna.gz".  Returns the name's length, of which
 *                    min(length, cap) bytes are written to out; negative: an error code.
 * gs_asmsum_kernel_time  profile != 0: from now on scan and finish run between events; what they add up to so far.
 * NULL or negative arguments: GS_E_INVALID, before any device call.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_asmsum gs_asmsum;
typedef struct {
    int32_t n_nodes;
    const int32_t *known_taxids;
    const uint8_t *filter;
    int32_t quality_mask;
    int32_t reference_only, use_species_taxid;
    int64_t reserve_entries;
} gs_asmsum_cfg;
int gs_asmsum_create(gs_asmsum **out, int device, const gs_asmsum_cfg *cfg);
int gs_asmsum_submit(gs_asmsum *as, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t report[8]);
int gs_asmsum_append(gs_asmsum *as, const int32_t *nodes, const uint8_t *quality, const uint8_t *is_ref, const int64_t *lines,
                     const uint64_t *str_off, const uint8_t *pool, int64_t n, int64_t n_counted, int64_t n_lines);
int gs_asmsum_finish(gs_asmsum *as, int32_t max_per_node, int64_t info[4]);
int gs_asmsum_fetch(gs_asmsum *as, int32_t *nodes, uint8_t *quality, uint8_t *is_ref, int64_t *lines, uint64_t *str_off, uint8_t *pool);
int64_t gs_asmsum_file_name(const uint8_t *ftp, int64_t n, uint8_t *out, int64_t cap);
int gs_asmsum_get_device(gs_asmsum *as, int *device);
int gs_asmsum_kernel_time(gs_asmsum *as, int profile, int64_t *launches, double *total_ms);
int gs_asmsum_destroy(gs_asmsum *as);

/* ---------------------------------------------------------------------------------------------------
 * taxtree: NCBI nodes.dmp / names.dmp to the arrays of the tree, the taxnodes selection and the tree a database carries
 * (genestrip_amd/csrc/gs_taxtree.hip, genestrip_amd/csrc/gs_taxparse.h)
 *
 * Replaces TaxTree(File, boolean) (C/tax/TaxTree.java:92-122, readNodesFromStream :226-254, readNamesFromStream :196-216,
 * initPositions :491-502), TaxIdCollector.withDescendants under TaxNodesGoal (C/tax/TaxIdCollector.java:119-126,172-185,
 * C/goals/TaxNodesGoal.java:74-94) and markRequired / SmallTaxTree(TaxTree) / Database.initStoreIndices (TaxTree.java:536-544,
 * C/tax/SmallTaxTree.java:60-64,427-454, C/store/Database.java:107-128; the value indices are those of a store that has no values
 * yet, and nothing else).  What the reference does on every kind of line is stated at the head of gs_taxparse.h, the grammar
 * inside which the device takes a chunk of nodes lines at the head of gs_taxtree.hip.
 *
 * A node is its index in the ascending array of distinct tax ids -- of first fields and of parents: a parent that no line
 * introduces is a node without rank and parent.  gs_taxtree_fetch's taxids are the known_taxids of gs_accmap_create.  The
 * reference keys nodes by the string of the id; here a tax id is 1-9 digits without a leading zero, and a line whose id or parent
 * is anything else made of digits fails with GS_E_UNSUPPORTED.  Where the reference throws, the call fails with GS_E_INVALID and
 * names the 1-based line.
 *
 * gs_taxtree_create        device -1: a HOST-ONLY tree: it touches no device, takes lines through the append calls alone
 *                          (gs_taxtree_submit_nodes: GS_E_UNSUPPORTED), builds the reference's child lists and walks them without
 *                          recursion, and answers every call below from host memory (mem: GS_MEM_HOST alone).
 * gs_taxtree_submit_nodes  text: n_bytes (at most 1 GiB) of whole nodes lines in host or device memory, free again on return.
 *                          last != 0: the stream ends here and its final line need not be terminated.  report: [0] lines,
 *                          [2] slots taken (one per line), [3] 1: REFUSED -- the handle is as it was and the caller owes the
 *                          chunk to gs_taxtree_append_nodes, [4] the first line outside the grammar (0-based in the chunk; -1:
 *                          none), [5] the longest line with its newline, [1] [6] [7] 0.
 * gs_taxtree_append_nodes  the same lines judged one by one on the host, at their place in the input order.  report: [0] lines as
 *                          the reference counts them (a line beyond 4096 bytes is two), [2] lines that were not skipped.  A
 *                          failure leaves the handle as it was.
 * gs_taxtree_finish_nodes  the tree: distinct ids, parents by search, child lists by one stable sort of (parent, line), depth,
 *                          pre-order position and subtree size by pointer jumping over the Euler tour -- a number of launches
 *                          that grows with log(nodes), not with the depth.  A node that the root does not reach (another
 *                          self-parent node, a parent-only node, a cycle, and what hangs below them) has depth -1, position -1,
 *                          subtree 0.  No line with id 1 and parent 1: GS_E_INVALID, "no root".  info: [0] nodes, [1] nodes the
 *                          root reaches, [2] the deepest of them, [3] lines whose id had a line before -- the device's finish
 *                          cannot say what the reference does with those (the node is listed twice and keeps its last parent),
 *                          so the handle then builds the host's lists and [4] is 1: the tree lives on the host from here on,
 *                          as it does on a host-only handle; [5] nodes on a cycle of parent links, [6] slots, [7] 0.
 * gs_taxtree_submit_names  text: whole names lines in host or device memory, behind gs_taxtree_finish_nodes, scanned on the device
 *                          inside the names grammar at the head of gs_taxtree.hip.  A node takes the name of the first line
 *                          that names it, and of every later line that holds "scientific name" anywhere: one 64-bit atomicMax
 *                          per line decides among the lines of the whole stream, and the names of a chunk's winners are
 *                          gathered into a pool on the device before the call returns.  report as for
 *                          gs_taxtree_submit_nodes; a REFUSED chunk wrote nothing and goes to gs_taxtree_append_names.  A tree
 *                          that lives on the host: GS_E_UNSUPPORTED.
 * gs_taxtree_append_names  the same lines judged one by one on the host, at their place in the input order (line numbers run
 *                          through both calls, so a scientific line of either beats a synonym of the other).
 * gs_taxtree_fetch         host arrays of n nodes each, any of them NULL: taxids, parent (node index; -1), depth, position,
 *                          subtree, rank (ordinal of C/tax/Rank.java; -1).
 * gs_taxtree_fetch_names   offsets[n + 1]: where the name of node i starts in bytes, or -1 - that if it has none;
 *                          offsets[n]: the bytes in all.  bytes NULL: the offsets alone.  Names are the bytes of the line (the
 *                          reference decodes them as UTF-8).
 * gs_taxtree_select        the taxnodes set: requested and excluded are node indices (host); cut_rank is the ordinal of
 *                          rankCompletionDepth or -1.  out[n] (host): 1 for a node of withDescendants(requested, cut) that is
 *                          not in withDescendants(excluded, null); *count (may be NULL): how many.  Descent follows child lists
 *                          whether the root reaches them or not.  A requested or excluded node on a cycle: GS_E_INVALID (the
 *                          reference's recursion does not end).
 * gs_taxtree_small         flagged[n]: uint8 (flag_bytes 1) or int32 (flag_bytes 4; > 0 means flagged: the regions of
 *                          gs_accmap_fetch), host or device memory.  The nodes the root reaches that are flagged or have a
 *                          flagged descendant, and the root, in pre-order: *n_small and, per value index, node_of_vi, parent_vi
 *                          (-1 for the root: what gs_dbbuild_begin takes), depth, position (host, room for info[1] entries; any
 *                          may be NULL).  position is the FULL tree's, as SmallTaxTree's constructor copies it.
 * gs_taxtree_regions_below the taxfromgenbank set (C/goals/genbank/TaxNodesFromGenbankGoal.java:86-92).  regions[n]: entries of the
 *                          accession map per node ITSELF, as gs_accmap_fetch gives them, host or device memory (host: a negative
 *                          count is GS_E_INVALID; device: taken as it is).  The count the goal compares is the one of
 *                          TaxIdNode.incRefSeqRegions (C/tax/TaxTree.java:517-521): the entries whose node is this node or has it
 *                          on its parent chain.  For the nodes the root reaches the device scatters regions to pre-order, scans
 *                          once and takes the difference over [position, position + subtree); what the root does not reach, a
 *                          tree that lives on the host and a host-only tree walk parents on the host.  Sums are kept mod 2^32, so
 *                          a count below 2^31 is exact.  A node with regions on or below a cycle of parent links: GS_E_INVALID
 *                          (the reference's walk does not end).  selected: n_selected node indices (host; the taxnodes set).
 *                          inclusive[n] (host, may be NULL): the count per node.  below (host, room for n_selected, may be NULL)
 *                          and *n_below (may be NULL): the selected nodes with rank == check_rank (-1: any rank) and
 *                          inclusive < limit, once each, in ascending node index (the reference's set has no order).  What the
 *                          goal puts in front stays with the caller: without refseq.filldb the set is the whole selection; with
 *                          SeqType.RNA, or with limit <= 0, it is empty (:74-84).
 * gs_taxtree_read_taxids   TaxIdCollector.readFromFile over the bytes of a tax id file: the ids (1-9 digits) of requested and
 *                          of '-' lines; at most cap of each are written, the counts say how many there are.
 * gs_taxtree_finish_times  ms[3] of the last finish between events, if profiling was on: distinct ids and parents (one key sort, one
 *                          scan, the searches) | child order (one pair sort) | tree steps (Euler tour, jumping, cycles); zeros else.
 * gs_taxtree_kernel_time   profile != 0: from now on scan, finish, select and small run between events; what they add up to.
 * NULL or negative arguments: GS_E_INVALID, before any device call.  Calls out of order: GS_E_STATE.
 * ------------------------------------------------------------------------------------------------- */
typedef struct gs_taxtree gs_taxtree;
int gs_taxtree_create(gs_taxtree **out, int device);
int gs_taxtree_submit_nodes(gs_taxtree *t, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t report[8]);
int gs_taxtree_append_nodes(gs_taxtree *t, const uint8_t *text, int64_t n_bytes, int last, int64_t report[8]);
int gs_taxtree_finish_nodes(gs_taxtree *t, int64_t info[8]);
int gs_taxtree_submit_names(gs_taxtree *t, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t report[8]);
int gs_taxtree_append_names(gs_taxtree *t, const uint8_t *text, int64_t n_bytes, int last);
int gs_taxtree_fetch(gs_taxtree *t, int32_t *taxids, int32_t *parent, int32_t *depth, int32_t *position, int32_t *subtree, int32_t *rank);
int gs_taxtree_fetch_names(gs_taxtree *t, int64_t *offsets, uint8_t *bytes, int64_t cap);
int gs_taxtree_select(gs_taxtree *t, const int32_t *requested, int64_t n_requested, const int32_t *excluded, int64_t n_excluded, int cut_rank,
                      uint8_t *out, int64_t *count);
int gs_taxtree_small(gs_taxtree *t, const void *flagged, int flag_bytes, int mem, int32_t *n_small, int32_t *node_of_vi, int32_t *parent_vi,
                     int32_t *depth, int32_t *position);
int gs_taxtree_regions_below(gs_taxtree *t, const int32_t *regions, int mem, const int32_t *selected, int64_t n_selected, int32_t limit, int check_rank,
                             int32_t *inclusive, int32_t *below, int64_t *n_below);
int gs_taxtree_read_taxids(const uint8_t *text, int64_t n_bytes, int32_t *requested, int64_t *n_requested, int32_t *excluded, int64_t *n_excluded,
                           int64_t cap);
int gs_taxtree_get_device(gs_taxtree *t, int *device);
int gs_taxtree_finish_times(gs_taxtree *t, double ms[3]);
int gs_taxtree_kernel_time(gs_taxtree *t, int profile, int64_t *launches, double *total_ms);
int gs_taxtree_destroy(gs_taxtree *t);

#ifdef __cplusplus
}
#endif
#endif
