/*
 * gshost.h -- C++ host layer above the C ABI (libgshost.so): the pieces of the reference's Java host that sit
 * directly on either side of the hot path, written natively because the reference's toolchain (JDK) is absent
 * here and its host is compiled code.  It is what a no-JVM deployment (or the test-suite) drives; the Java host of
 * INTEGRATION.md keeps using its own parser/reporter and only needs include/gsgpu.h.
 *
 *   gs_fastq_*            FASTQ / FASTA ingest with the reference's exact record semantics
 *                         (C/fastq/AbstractFastqReader.java:288-438 over B/io/BufferedLineReader.java:114-182;
 *                         gzip by file suffix, B/io/StreamProvider.java:92-100,148-150), batched for gs_match_submit
 *   gs_host_match_files   FastqKMerMatcher.runMatcher (C/match/FastqKMerMatcher.java:181-235): files -> batches ->
 *                         GPU -> per-taxid table, totals, optional filtered FASTQ (:304-307) and Kraken-style
 *                         output (:308-314, :723-756); parsing of batch i+1 overlaps the GPU work of batch i
 *   gs_host_filter_files  FastqBloomFilter.runFilter (C/bloom/FastqBloomFilter.java:80-105)
 *   gs_host_write_csv     MatchingResult.completeResults + ResultReporter.printMatchResult
 *                         (C/match/MatchingResult.java:84-118, C/match/ResultReporter.java:190-279)
 *   gs_host_kraken_count_files  the krakencount goal: Kraken-style output files -> reads / k-mers per tax id
 *   gs_host_write_quality_csv  the dbquality goal's CSV (DBQualityCountsGoal's rank aggregation + DBQualityCSVGoal.makeFile)
 *   gs_host_genome_files  genome FASTA files -> the regions of a build (the walk of AbstractFastaReader.readFasta under the
 *                         store readers), records found and bases gathered on the device, the selection left to a callback
 *   gs_host_genome_files_into  the same without callbacks: accession map, a table of value indices per node, one of the four region
 *                         handles as the target -- what the JNI shim binds
 *   gs_host_control_*     progress records and cancellation of the file-level calls above (ExecutionContext.setFastqProgress /
 *                         setTotalProgress, FastqReaderInterruptedException), through a control attached to the calling thread
 * (C/ = core/src/main/java/org/metagene/genestrip/, B/ = base/src/main/java/org/metagene/genestrip/)
 */
#ifndef GSHOST_H
#define GSHOST_H

#include "gsgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- FASTQ / FASTA reader ---- */
typedef struct gs_fastq gs_fastq;

typedef struct {
    int64_t n_reads;
    const uint8_t *seq;        /* concatenated reads                                   */
    const uint64_t *seq_off;   /* n_reads + 1                                          */
    const uint8_t *desc;       /* descriptors incl. the leading '@' (FASTA: rewritten) */
    const uint64_t *desc_off;
    const uint8_t *qual;       /* quality bytes; FASTA: empty                          */
    const uint64_t *qual_off;
    int64_t first_read_no;     /* 0-based index of the first read within its file      */
} gs_read_batch;

/* fasta: 0 = FASTQ, 1 = FASTA, -1 = decide by suffix (.fasta/.fa/.fna/.fas[.gz|.gzip], C/goals/FastqMapGoal.java:188-201) */
int gs_fastq_open(gs_fastq **out, const char *path, int fasta, int k);
/* next batch of at most max_reads reads / max_bytes sequence bytes; n_reads == 0 at end of file.
 * The pointers stay valid until the next call on the same reader. */
int gs_fastq_next(gs_fastq *r, int64_t max_reads, int64_t max_bytes, gs_read_batch *batch);
/* totals so far: reads, k-mers (sum of max(0, L-k+1)), base pairs (AbstractFastqReader.java:343-349) */
int gs_fastq_totals(const gs_fastq *r, int64_t *reads, int64_t *kmers, int64_t *bps);
int gs_fastq_close(gs_fastq *r);

/* ---- runMatcher ---- */
typedef struct {
    const char *filtered_path;     /* reads with matchRead() == true, rewritten like ReadEntry.write; NULL = off;
                                      gzip when the name ends in .gz/.gzip                                     */
    const char *kraken_out_path;   /* Kraken-style per-read lines; NULL = off                                  */
    int32_t write_all;             /* writeAll: also lines of unclassified reads (C/GSConfigKey.java:315)      */
    const char *const *taxids;     /* taxid string per value index (needed for the Kraken-style output)        */
    int64_t batch_reads;           /* 0 = default (1 Mi reads)                                                 */
    int32_t with_probs;            /* withProbs (C/GSConfigKey.java:364): written reads keep their quality line(s)
                                      (ReadEntry.write, AbstractFastqReader.java:570-584) instead of '~' x length */
    uint8_t *max_contig_desc;      /* NULL, or n_values x max_contig_desc_stride bytes: per value index the name of the read
                                      that holds the longest contig (CountsPerTaxid.maxContigDescriptor, FastqKMerMatcher.java
                                      :401-407: the descriptor behind its first character up to the first blank), NUL-terminated,
                                      cut to fit; empty when there is none.  Costs one synchronisation per chunk.  Reads of FASTA /
                                      multi-line FASTQ chunks that the device parsed leave the name empty.              */
    int32_t max_contig_desc_stride;
} gs_host_match_opts;

typedef struct {
    int64_t reads, kmers, bps;     /* totalReads / totalKMers / totalBPs                                        */
    int64_t filtered_reads;        /* reads written to filtered_path                                            */
    double seconds_total, seconds_parse, seconds_gpu;
} gs_host_totals;

/* processes the files in order with ONE gs_run (begin..finish); table/dtable as gs_match_finish */
int gs_host_match_files(gs_db *db, const gs_match_cfg *cfg, const char *const *paths, int n_paths,
                        const gs_host_match_opts *opts, int64_t *table, double *dtable, gs_host_totals *totals);

/* The same into a run the caller began and will finish (gs_match_begin ... gs_match_finish), per-read outputs included: what a
 * host that keeps ONE run per matcher calls once per runMatcher -- java/src/.../match/GpuFastqKMerMatcher.java: a store allows one
 * unique-counting run at a time, and the matcher's own run is it.  Read numbers run over the files in order, from 0. */
int gs_host_match_run(gs_run *run, gs_db *db, const char *const *paths, int n_paths, const gs_host_match_opts *opts,
                      gs_host_totals *totals);

/* The files of a run into a gs_run that the caller began and will finish -- for one-process-per-GPU runs that share
 * the files of a sample (genestrip_amd/distributed.py: match_files_sharded): every process takes some of the files,
 * merges its run's device state with the others (gs_match_device_state) and finishes.  file_index[n_paths] = position
 * of each file in the global file order; read numbers on the device are (file_index << 32 | read in file), so the
 * max-contig tie-break keeps the global file order; reads_of_file[n_paths] receives the read counts, which turn those
 * numbers into running ones after the merge.  No per-read outputs.  file_index[i] must lie in [0, GS_HOST_MAX_FILE_INDEX)
 * (the max-contig key has 40 bits for the read number: 8 for the file, 32 for the read); GS_E_UNSUPPORTED otherwise. */
#define GS_HOST_MAX_FILE_INDEX 256
int gs_host_match_into(gs_run *run, gs_db *db, const char *const *paths, int n_paths, const int32_t *file_index,
                       int64_t *reads_of_file, gs_host_totals *totals);

/* runMatcher over the files of a sample on several devices of THIS process (what a JVM host with 8 GPUs calls):
 * dbs[d] = a replica of the store on device d (or the handles of ONE striped store, gs_db_create_striped); file i goes to replica i % n_dbs, every replica runs on a thread of its
 * own (as gs_host_match_into), the runs are merged with gs_match_merge (RCCL between devices) and finished once.  The
 * table equals the one gs_host_match_files returns for the same files in the same order.  No per-read outputs. */
int gs_host_match_files_multi(gs_db *const *dbs, int n_dbs, const gs_match_cfg *cfg, const char *const *paths, int n_paths,
                              int64_t *table, double *dtable, gs_host_totals *totals);

/* diagnostics: which = 0: chunks of text that went through the general (multi-line) FASTQ device path of the match goal in this
 * process so far; 1: FASTA / general FASTQ chunks that the filter goal handled on the device; 2: chunks of the match goal whose
 * Kraken-style lines were written on the device (gs_match_kraken_text; GS_DEVICE_KRAKEN=0 keeps them on the host; four-line chunks
 * only); 3: FASTA / general FASTQ chunks of any goal (match, filter, extract) whose per-read output -- filtered file, accepted / rest
 * file, selected records, Kraken-style lines -- was written on the device (gs_*_compact_records, gs_match_kraken_records;
 * GS_DEVICE_RECORDS=0 keeps them on the host); 5: chunks of Kraken-style lines that gs_host_kraken_count_files counted on the device (4 is no counter: -1) */
int64_t gs_host_stat(int which);

/* ---- runFilter: accepted reads -> filtered_path, the rest -> rest_path (either may be NULL); with_probs as above ---- */
int gs_host_filter_files(gs_bloom *bloom, int k, int min_pos_count, double positive_ratio, const char *const *paths,
                         int n_paths, const char *filtered_path, const char *rest_path, int with_probs,
                         gs_host_totals *totals);

/* ---- extract (C/goals/ExtractGoal.java:73-129): every read of the files (in order; FASTQ or FASTA by suffix; plain, gzip or BGZF)
 * whose descriptor behind its first byte starts with `key` (ByteArrayUtil.startsWith(readDescriptor, 1, key), :93) is written to
 * out_path as ReadEntry.write does with the goal's withProbs = true; a name ending in .gz / .gzip is written as BGZF.  Readers,
 * device inflaters and writers are those of gs_host_filter_files, the selection runs on the device (gs_reads_select_*); with
 * GS_HOST_FAST=0 everything goes through the reference-exact parser and no device is used.  An empty key or a byte >= 0x80 in
 * it: GS_E_INVALID.  totals: reads / kmers / bps as for the filter (k only feeds them), filtered_reads = reads written. ---- */
int gs_host_extract_files(int device, const char *key, int k, const char *const *paths, int n_paths, const char *out_path,
                          gs_host_totals *totals);

/* ---- fasta2fastq (C/goals/Fasta2FastqGoal.java:92-165): the FASTA files, in order, into ONE four-line FASTQ file with '~'
 * qualities (.gz / .gzip: BGZF).  Chunks of whole records are rewritten on the device (gs_reads_fasta2fastq); a record that does
 * not fit a chunk, a file that does not start with '>', a NUL byte or a byte >= 0x80 (the reference's PrintStream widens those),
 * the tail of a file without a final newline and everything under GS_HOST_FAST=0 (no device is used then) go through a plain loop
 * that follows the reference line by line.  A line of 65 534 bytes or more: GS_E_INVALID (the reference throws).  *n_records
 * (may be NULL) = header lines seen. ---- */
int gs_host_fasta2fastq(int device, const char *const *paths, int n_paths, const char *out_path, int64_t *n_records);

/* ---- db2fastq (C/goals/DB2FastqGoal.java, C/fastqgen/KMerFastqGenerator.java): the stored k-mers selected as by
 * gs_dbexport_create (sel_vi = -1: all -- the goal's "total" file; with_desc: the subtree of sel_vi -- a "taxid+" entry) written to
 * `path` in ascending k-mer order, one FASTQ record each as FastQWriter prints it (gs_dbexport_fastq_begin; taxids[n_values] =
 * SmallTaxIdNode.getTaxId per value index, project = the project name).  A name ending in .gz / .gzip is written as BGZF (gzip
 * members + the EOF block) compressed by the device DEFLATE writer, else plain text; the text is made on the device and crosses
 * to the host only as the file's bytes.  *n_written = records written. ---- */
int gs_host_db2fastq(gs_db *db, const char *const *taxids, const char *project, int32_t sel_vi, int with_desc, const char *path,
                     int64_t *n_written);

/* ---- completeResults + CSV ---- */
typedef struct {
    int32_t n_values;
    const int32_t *parent_vi;      /* as gs_db_create                                                   */
    const int32_t *position;       /* tree sort position per value index (SmallTaxIdNode position); NULL = pre-order */
    const char *const *taxids;
    const char *const *names;      /* may be NULL                                                       */
    const char *const *ranks;      /* Rank.toString() per node, may be NULL                             */
    const int64_t *db_kmers;       /* k-mers stored per value index (Database.getStats)                 */
    int64_t db_kmers_total;
    const char *const *max_contig_desc; /* per value index, may be NULL                                 */
    const int16_t *max_kmer_counts;     /* gs_match_max_counts output ((n_values+1) x max_kmer_res_counts) or NULL */
    int32_t max_kmer_res_counts;        /* > 0 adds the experimental "max kmer counts" column (pos 2001)          */
} gs_host_tax_info;

int gs_host_write_csv(const char *path, const gs_host_tax_info *tax, const int64_t *table, const double *dtable,
                      const gs_host_totals *totals);

/* ---- the dbquality goal's CSV (ft/src/main/java/org/metagene/genestrip/finertree/goals/DBQualityCountsGoal.java:149-173 with
 * Counts.aggregate and its getters, DBQualityCSVGoal.makeFile) from the output of gs_dbquality_finish (include/gsgpu.h):
 * counts[n_values][3] = tp, tp+fp, tp+fn and present[n_values].  Every present node, in tree order (ascending `position`,
 * pre-order when NULL), is aggregated into its nearest ancestor-or-self of each of the ranks "cellular root", "acellular root",
 * "species", "genus" that has no row of its own: the three counts are added, and the row's precision and recall sums gain the
 * child's values.  One line per node with a row, in tree order:
 *   taxid;name;rank;parent taxid;tp;tp+fp;tp+fn;precision;recall;weighted avg precision;weighted avg recall;
 * with `null` as the root's parent and the doubles as DecimalFormat("0.00000000") in Locale.US prints them.  As in the
 * reference the columns named precision / recall hold the UNWEIGHTED average over the aggregated nodes (a row of its own: tp /
 * (tp+fp), tp / (tp+fn)), the columns named weighted avg ... hold tp / (tp+fp) and tp / (tp+fn) of the added counts.  Of `tax`
 * only n_values, parent_vi, position, taxids, names and ranks are read. ---- */
int gs_host_write_quality_csv(const char *path, const gs_host_tax_info *tax, const int64_t *counts, const uint8_t *present);

/* ---- krakencount / krakenres (C/goals/kraken/KrakenResCountGoal.java:133-157 over C/kraken/KrakenResultProcessor.java:74-179;
 * the CSV of C/goals/kraken/KrakenResFileGoal.java:95-107): per tax id of Kraken-style output files -- ours, Kraken's,
 * KrakenUniq's -- the reads, the k-mers and the k-mers in matching reads.  Each file (plain or gzip, BGZF included) is one stream
 * under the reference's rules: it ends at its first empty line, an unterminated last line loses its last byte; all files go into
 * one table.  Chunks of whole lines are counted on the device (gs_krakencount); a chunk it refuses, the unterminated tail of a
 * file, a line that does not fit a block and everything under GS_HOST_FAST=0 (no device is used then) go through a line-by-line
 * restatement of the reference (genestrip_amd/csrc/gs_krakenparse.h); both give the same rows for every file.
 * only_taxids (n_only > 0): rows of other keys are dropped, as by the goal's tax id set.
 * Rows come in the order of DigitTrie.collect: keys[i * key_stride ..] NUL-terminated, counts[3 * i ..] = reads, kmers, kmers in
 * matching reads.  *n_rows is always set; rows are written if cap_rows >= *n_rows and every key fits key_stride, else the call
 * fails with GS_E_INVALID after the CSV (csv_path != NULL: gs_host_write_kraken_csv) has been written.
 * Two deliberate differences: a line of more than 65 536 bytes with its newline (the reference fails: array index) counts like any
 * other and is reported in long_lines; where the reference throws -- a non-digit in a count, a read size or a class -- the call
 * fails with GS_E_INVALID, gs_host_last_error() names the file and the 1-based line, and nothing is written. ---- */
typedef struct {
    int64_t lines, counted_tokens, a_tokens, long_lines;  /* lines read; tokens counted; 'A' tokens skipped; lines > 65 536 bytes */
    int64_t device_chunks, host_chunks;                   /* chunks the device counted; chunks and tails the line-by-line loop took */
    double seconds_total;
} gs_host_kraken_totals;
int gs_host_kraken_count_files(int device, const char *const *paths, int n_paths, const char *const *only_taxids, int n_only,
                               const char *csv_path, char *keys, int32_t key_stride, int64_t *counts, int64_t cap_rows, int64_t *n_rows,
                               gs_host_kraken_totals *totals);
/* taxid;reads;kmers;kmers in matching reads -- then key;reads;kmers;kimr; per row, '\n' line ends; .gz / .gzip: gzip */
int gs_host_write_kraken_csv(const char *path, const char *keys, int32_t key_stride, const int64_t *counts, int64_t n_rows);

/* ---- genome FASTA files to the regions of a build (the walk of AbstractFastaReader.readFasta that fillsize, tempindex / filldb,
 * updatedb and dbqualcounts each repeat): every file (plain or gzip, BGZF included), in order, is cut into chunks of whole records;
 * gs_genomes (include/gsgpu.h) finds the records of a chunk on the device, `resolve` sees their header lines and says per record
 * which value index it counts for (vi[i] < 0: skip -- accession map, tree, limits are the caller's), the bases of the kept records
 * are gathered on the device and handed to `sink` as (seq, off[n_regions + 1], vi[n_regions]) with vi compacted to the kept
 * regions: exactly what gs_dbsize_add / gs_dbbuild_add / gs_dbupdate_add / gs_dbquality_add take, with `mem` saying where seq and
 * off live.  They are valid until the sink returns.  A record longer than a reader block (GS_HOST_BLOCK_BYTES; this loop's default
 * is 64 MiB): the file goes on from that record with blocks twice as large, up to the 1 GiB a chunk may hold (a gzip stream is
 * inflated from its start again, what has been worked off is passed over); a record beyond that size, with the rest of its file,
 * goes through a line-by-line restatement of the reference
 * (genestrip_amd/csrc/gs_genomeparse.h), as do a chunk the device refuses (a NUL byte, a run of more than 64 '\r') and everything
 * under GS_HOST_FAST=0 (no device is used then); they reach the same sink with mem = GS_MEM_HOST.  first_record counts the records of `file` (an index into paths) in front of the batch.  A callback's
 * non-zero return ends the walk and is returned (positive codes keep it apart from the GS_E_* codes of the call itself).  Blocks are read and gzip is inflated by the threads of the text readers the
 * other goals use; the text of a chunk is staged to the device by gs_genomes_scan. ---- */
typedef int (*gs_genome_resolve_fn)(void *user, int file, int64_t first_record, int64_t n_records, const uint8_t *headers,
                                    const uint64_t *header_off, int32_t *vi);
typedef int (*gs_genome_sink_fn)(void *user, const uint8_t *seq, const uint64_t *off, const int32_t *vi, int64_t n_regions, int mem);
typedef struct {
    int64_t records, kept_records;       /* records seen; records the resolver kept                                        */
    int64_t text_bytes, kept_bases;      /* bytes of FASTA text walked; bases handed to the sink                           */
    int64_t chunks, host_chunks;         /* chunks in all; chunks (and rests of files) the line-by-line parser took        */
    int64_t max_line_bytes;              /* the longest line with its newline (the reference throws from fastaLineSizeBytes - 1 on) */
    double seconds_total;
} gs_host_genome_totals;
int gs_host_genome_files(const char *const *paths, int n_paths, int device, gs_genome_resolve_fn resolve, void *resolve_user,
                         gs_genome_sink_fn sink, void *sink_user, gs_host_genome_totals *totals);

/* The accmapsize / accmap goals over RefSeq catalog files (AccessionFileProcessor.processCatalog, C/refseq/AccessionFileProcessor.java
 * :96-131, under AccessionMapSizeGoal / AccessionMapGoal): every file (plain or gzip, BGZF included) is one stream, all of them go into
 * one map.  Chunks of whole lines are scanned on the device (gs_accmap_submit, include/gsgpu.h); a chunk the device refuses, a line that
 * does not fit a reader block with the rest of its file, the unterminated tail of a file and, under GS_HOST_FAST=0, everything go
 * through the line-by-line restatement of the reference (genestrip_amd/csrc/gs_accmapparse.h), whose entries join the map in input
 * order (gs_accmap_append).  Under GS_HOST_FAST=0 no device is used and *out is a host-only map (device -1: fetch and host lookups).
 * count_only != 0 is the accmapsize goal: totals->passing is its number, no map is kept, *out is NULL (out may be NULL).  Otherwise
 * *out is the finished map, the caller's to destroy.  Where the reference throws -- a line that does not fit its 2048-byte buffer, the
 * put of an entry of two tabs -- the call fails with GS_E_INVALID and gs_host_last_error names the file and the 1-based line; an
 * accession of more than 31 bytes, or with a byte from 0x80 on, in an entry that is put fails with GS_E_UNSUPPORTED naming it (RefSeq
 * has none).  Progress records count lines; on GS_E_CANCELLED no map is returned. */
typedef struct {
    int64_t lines, passing, put;         /* lines read; entries that pass (the accmapsize number); entries put into the map */
    int64_t device_chunks, host_chunks;  /* chunks the device scanned; chunks (and rests of files) the line-by-line parser took */
    double seconds_total;
} gs_host_accmap_totals;
int gs_host_accmap_files(const char *const *paths, int n_paths, int device, const gs_accmap_cfg *cfg, int count_only, gs_accmap **out,
                         gs_host_accmap_totals *totals);

/* The fastasgenbank goal over Genbank assembly summary files (AssemblySummaryReader.getRelevantEntries, C/genbank/
 * AssemblySummaryReader.java:104-144, under the cap of FastaFilesFromGenbankGoal, C/goals/genbank/FastaFilesFromGenbankGoal.java:101-150):
 * every file (plain or gzip, BGZF included) is one stream, all of them go into one handle, and a line's number counts the lines of the
 * files in front of it too.  Chunks of whole lines are judged on the device (gs_asmsum_submit, include/gsgpu.h); a chunk the device
 * refuses (a CR, a line above 4096 bytes, a byte from 0x80 on in a key field), a line that does not fit a reader block with the rest of
 * its file, the unterminated tail of a file and, under GS_HOST_FAST=0, everything go through the record-by-record restatement of the
 * reference (genestrip_amd/csrc/gs_asmsumparse.h), whose entries join the handle in input order (gs_asmsum_append).  Under
 * GS_HOST_FAST=0 no device is used and *out is a host-only handle (device -1).  *out is the finished handle (gs_asmsum_finish with
 * max_per_node; gs_asmsum_fetch gives the picks), the caller's to destroy.  Where the reference throws -- a kept entry with an empty ftp
 * path -- the call fails with GS_E_INVALID and gs_host_last_error names the file and the 1-based line of that file.  Progress records
 * count lines; on GS_E_CANCELLED no handle is returned.  The goal's early exit (an empty taxfromgenbank set: no file is read) is the
 * caller's. */
typedef struct {
    int64_t lines, counted, kept;        /* lines read; records of 20 fields and more; entries kept in front of the cap */
    int64_t picked, nodes;               /* entries behind the cap; nodes with entries */
    int64_t device_chunks, host_chunks;  /* chunks the device judged; chunks (and rests of files) the record-by-record parser took */
    double seconds_total;
} gs_host_asmsum_totals;
int gs_host_asmsum_files(const char *const *paths, int n_paths, int device, const gs_asmsum_cfg *cfg, int32_t max_per_node, gs_asmsum **out,
                         gs_host_asmsum_totals *totals);

/* The taxtree goal over an NCBI taxonomy dump (TaxTree(File, boolean), C/tax/TaxTree.java:92-122): nodes_path (nodes.dmp) and, unless
 * NULL, names_path (names.dmp), each plain or gzip, BGZF included.  Chunks of whole nodes lines are scanned on the device
 * (gs_taxtree_submit_nodes, include/gsgpu.h); a chunk the device refuses, a line that does not fit a reader block with the rest of its
 * file, the unterminated tail and, under GS_HOST_FAST=0, everything go through the line-by-line restatement of the reference
 * (genestrip_amd/csrc/gs_taxparse.h) at their place in the input order (gs_taxtree_append_nodes).  names.dmp goes the same way through
 * gs_taxtree_submit_names / _append_names.  Under GS_HOST_FAST=0 no device is used and *out is a host-only tree (device -1).  *out is the finished
 * tree, the caller's to destroy.  Where the reference throws the call fails with GS_E_INVALID, a tax id that is no 1-9 digits without a
 * leading zero with GS_E_UNSUPPORTED, and gs_host_last_error names the file and the 1-based line.  Progress records count lines; on
 * GS_E_CANCELLED no tree is returned.  report: [0] nodes lines, [1] names lines, [2] chunks the device scanned, [3] chunks (and rests
 * of files) that went line by line, [4] nodes, [5] nodes the root reaches, [6] lines whose id had a line before, [7] 1: the tree lives
 * on the host (GS_HOST_FAST=0, or duplicate ids). */
int gs_host_taxtree_files(int device, const char *nodes_path, const char *names_path, gs_taxtree **out, int64_t report[8]);

/* TaxIdCollector.readFromFile (C/tax/TaxIdCollector.java:67-108) over a tax id file, plain or gzip: the tax ids (1-9 digits without a
 * leading zero; any other value names no node and is dropped) of the requested and of the '-' lines, in file order; at most cap of
 * each are written, the counts say how many there are. */
int gs_host_read_taxids_file(const char *path, int32_t *requested, int64_t *n_requested, int32_t *excluded, int64_t *n_excluded, int64_t cap);

/* gs_host_genome_files with an accession map in front of the resolver: the header lines of a chunk are looked up where the scan left
 * them (gs_accmap_lookup_genomes; a chunk that went through the host parser: gs_accmap_lookup on its header lines, the same rule), and
 * `resolve` gets node[n_records] (-1: none; AbstractRefSeqFastaReader.updateNodeFromInfoLine with completeGenomesOnly = complete_only)
 * instead of header text and answers vi[] as before.  The same walk, totals, progress and cancellation.  am: a finished map; with
 * GS_HOST_FAST=0 a host-only one. */
typedef int (*gs_genome_resolve_nodes_fn)(void *user, int file, int64_t first_record, int64_t n_records, const int32_t *node, int32_t *vi);
int gs_host_genome_files_mapped(const char *const *paths, int n_paths, int device, gs_accmap *am, int complete_only,
                                gs_genome_resolve_nodes_fn resolve, void *resolve_user, gs_genome_sink_fn sink, void *sink_user,
                                gs_host_genome_totals *totals);

/* gs_host_genome_files_mapped without callbacks, for the common case in which they do what a table can do -- and the form a host
 * behind a foreign-function layer without upcalls (the JNI shim) can call.  It is that call's loop with a resolver and a sink built in:
 * chunking, device scan, lookup where the scan left the header lines, host-parser fallbacks, GS_HOST_FAST=0, totals, progress and
 * cancellation are the same code.
 *   node_of_file[n_paths] or NULL: >= 0: every record of that file counts for that node, no lookup (ignoreAccessionMap of the additional
 *     FASTA files, C/goals/FastaReaderGoal.java:140-145); < 0 (and NULL): its records are looked up in `am` as above.
 *   vi_of_node[n_nodes]: the value index per tree node, < 0: skip the record (the taxNodes test of AbstractRefSeqFastaReader.infoLine,
 *     C/refseq/AbstractRefSeqFastaReader.java:180, as a table).  A record whose node is -1 is skipped.
 *   kind / handle: where the kept regions go -- gs_dbsize_add, gs_dbbuild_add (with `update`), gs_dbupdate_add or gs_dbquality_add of
 *     the handle, with the memory kind the loop delivers (device memory for chunks the device scanned).  A failing _add ends the walk and
 *     its code is returned; gs_host_last_error carries its message.
 * am: a finished map, or NULL if no file needs a lookup.  Checked before any device call, GS_E_INVALID: a file that needs a lookup
 * while am is NULL; n_nodes other than the map's (gs_accmap_get_n_nodes); a node_of_file entry >= n_nodes; an unknown kind; a NULL
 * handle, paths or (n_nodes > 0) vi_of_node.
 * NOT served: maxGenomesPerTaxid / maxKMersPerTaxid / maxPerTaxidRank (the limits of AbstractStoreFastaReader) and idNodes / fileNodes /
 * dataNodes (the finer-node options): a caller that configures any of them keeps gs_host_genome_files_mapped or its own reader. */
enum { GS_HOST_INTO_SIZE = 0, GS_HOST_INTO_BUILD = 1, GS_HOST_INTO_UPDATE = 2, GS_HOST_INTO_QUALITY = 3 };
int gs_host_genome_files_into(const char *const *paths, int n_paths, int device, gs_accmap *am, int complete_only,
                              const int32_t *node_of_file, const int32_t *vi_of_node, int32_t n_nodes, int kind, void *handle, int update,
                              gs_host_genome_totals *totals);

/* ---- progress and cancellation of the file-level calls (what the reference does through ExecutionContext.setFastqProgress /
 * setTotalProgress, C/fastq/AbstractLoggingFastqStreamer.java:161-209,247-252, and FastqReaderInterruptedException).
 * A control is attached to a THREAD (gs_host_control_attach); the file-level calls that thread makes afterwards -- gs_host_match_files,
 * _match_run, _match_into, _filter_files, _extract_files, _fasta2fastq, _kraken_count_files, _genome_files, _genome_files_mapped,
 * _genome_files_into, _accmap_files, _asmsum_files, _taxtree_files -- publish records to it and
 * look at its cancel flag after every chunk.  Their signatures are unchanged, and a thread without a control behaves as before.
 * Records: one at the start of each file (file_bytes_done = 0), one after every chunk or batch whose results are in the handle's
 * state, a last one per file (file_done = 1, file_bytes_done == file_bytes_total) and a closing one (files_done == n_files).  Files
 * read side by side interleave their records; `file` says whose a record is.  The match goal without per-read outputs keeps up to two
 * chunks on the device and looks for a refusal (text that is not what it was submitted as) only now and then: its chunk records count
 * the chunks SUBMITTED.  Should the device refuse one later, the chunk and those behind it are parsed again on the host and the count
 * stands still meanwhile; the record of a stop is exact all the same and may then report fewer reads than a record before it.
 * file_bytes_done counts bytes of the file as stored and
 * never decreases; for block-gzip input inflated on the device it is the offset of the next member, for other gzip streams -- whose
 * decoders run ahead of the loop on threads of their own -- an estimate (text / 4, kept below the file's size until the file is
 * through).  The callback runs on the calling thread, inside the call, never concurrently with itself; every_ms > 0 drops calls that
 * come sooner than that after the last, but never a file's first or last record, the closing record or the record of a stop.  The
 * snapshot follows every record.
 * A stop (the callback returned non-zero, or gs_host_control_cancel from any thread): nothing more is submitted, what is on the device
 * completes, writer / reader / inflating threads are joined, one more record gives the final counts (none behind a file's last record
 * or the closing one, when the stop was the answer to that: it holds them already) -- published before any
 * page-locked block, device text or pooled decoder is released -- and the call returns GS_E_CANCELLED with its totals filled.  The
 * state covers exactly the reads of that record, per file a prefix of the file's reads under the numbers they would have had; output
 * files are closed and hold exactly those reads' output (a .gz output ends at a member boundary, with its end-of-file block).
 * gs_host_match_run / _into leave the run usable (gs_match_finish: the table over those reads; gs_match_reset clears it);
 * gs_host_match_files runs its finish and fills table / dtable, gs_host_kraken_count_files fetches its rows (no CSV is written), the
 * sink of gs_host_genome_files has seen exactly the records reported.
 * Out of scope: gs_host_match_files_multi (its replicas run on threads of their own) and gs_host_db2fastq ignore an attached control;
 * the JNI shim's direct buffers are not bounds-checked (the stand-in jni.h has no GetDirectBufferCapacity). ---- */
typedef struct {
    int32_t file, n_files;        /* index of the file this record is about, and how many the call has      */
    int32_t file_done;            /* 1: the last record of this file                                          */
    int32_t files_done;           /* files completed so far                                                   */
    int64_t file_bytes_done, file_bytes_total;   /* bytes of the file as stored (compressed, if it is)        */
    int64_t file_reads;           /* reads (records, lines: the unit of the goal) of this file in the state   */
    int64_t total_bytes_done, total_bytes_total, total_reads;
    double  seconds_file, seconds_total;
} gs_host_progress;
typedef int (*gs_host_progress_fn)(void *user, const gs_host_progress *p);   /* non-zero: cancel */
typedef struct gs_host_control gs_host_control;
/* fn may be NULL (snapshots and the flag only).  A NULL or destroyed handle: GS_E_INVALID from every call below. */
int gs_host_control_create(gs_host_control **out, gs_host_progress_fn fn, void *user, int32_t every_ms);
int gs_host_control_destroy(gs_host_control *c);   /* a call that runs with it keeps it alive until it returns */
int gs_host_control_cancel(gs_host_control *c);                              /* any thread                    */
int gs_host_control_snapshot(gs_host_control *c, gs_host_progress *out, int32_t *cancelled);  /* any thread */
int gs_host_control_attach(gs_host_control *c);   /* this thread's file-level calls use c until detached; NULL detaches */

/* The host layer keeps page-locked blocks and the device decoders of gzip input (gigabytes of HBM) from call to call; this hands
 * them back (a long-lived JVM host before it loads a big store).  No other thread may be inside the host layer meanwhile. */
int gs_host_release_pools(void);

/* message of the last failure raised inside the host layer itself (failures of the C ABI: gs_last_error) */
const char *gs_host_last_error(void);

/* The ingest path's own gzip decoder (genestrip_amd/csrc/gs_inflate.h; replaces java.util.zip.GZIPInputStream,
 * B/io/StreamProvider.java:92-100) on a memory range, `block` output bytes per decode call -- exposed for the tests:
 * out receives the concatenated members; GS_E_INVALID for a corrupt stream (CRC-32 and ISIZE are checked). */
int gs_host_gunzip(const uint8_t *in, size_t n_in, uint8_t *out, size_t out_cap, size_t *n_out, size_t block);
/* ... and through the multi-threaded decoder of the gzip text path (speculative starts inside the stream, checked and
 * repaired by the in-order resolver): `threads` workers on compressed chunks of `chunk` bytes */
int gs_host_gunzip_parallel(const uint8_t *in, size_t n_in, uint8_t *out, size_t out_cap, size_t *n_out, int threads,
                            size_t chunk, size_t block);

/* Double.toString(double) -- exposed for the tests of the CSV writer */
int gs_host_java_double(double v, char *buf, int cap);

#ifdef __cplusplus
}
#endif
#endif
