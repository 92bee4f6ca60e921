// gs_launch.h -- the internal interface between the translation units of libgsgpu.so: every kernel launcher and every kernel
// parameter block that crosses a file boundary is declared here, once, and seen by its definer and by its callers alike.  Not
// part of the C ABI (include/gsgpu.h).  Declarations only: no inline functions (but the typed gs_dev_alloc), no state.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gs_params.h"

typedef unsigned long long u64;

// ---- parameter blocks (the ones of gs_kernels.hip, gs_route.hip, gs_segments.hip, gs_filter.hip and gs_text.hip: gs_params.h)
struct GsExportParams {
    const u64 *rec;        // this handle's record lines (GS_REC_WORDS words each), n_rec of them
    int64_t n_rec;
    const u64 *tab;        // this handle's table buckets (GS_SLOTS_PER_BUCKET slots each): global buckets tab_first ..
    int64_t tab_first, n_tab;
    uint32_t bucket_bits, vbits;
    int32_t k, n_values;
    const int32_t *tin, *tout;
    int32_t sel_vi;        // -1: every k-mer
    int32_t with_desc;     // 0: value == sel_vi, else tin[sel_vi] <= tin[value] < tout[sel_vi]
    u64 *count;            // k-mers emitted so far (one atomic per wave)
    u64 *keys;             // nullptr: count only
    uint32_t *vals;
    u64 cap;               // room in keys / vals
    u64 *hist;             // per value index, or nullptr
};

struct GsFastqParams {
    const u64 *keys;
    const uint32_t *vals;
    int64_t first, n;            // records [first, first + n) of the export
    int32_t k;
    const uint8_t *project;      // project_len bytes
    int32_t project_len;
    const uint8_t *names;        // taxid of value v: names[name_off[v] .. name_off[v + 1])
    const uint32_t *name_off;
    uint32_t *len;               // n + 1 record lengths (the last one 0) ...
    uint32_t *off;               // ... and their exclusive prefix: where each record starts, off[n] = the text's size
    uint8_t *text;
};

struct GsQualityParams {
    const u64 *keys;       // n pairs, ascending by (k-mer, leaf)
    const uint32_t *leaf;  // leaf value index, n_values = "counts nothing"
    int64_t n;
    const u64 *skeys;      // the m stored k-mers, ascending
    const uint32_t *svals;
    int64_t m;
    const int32_t *tin, *tout;
    int32_t n_values;
    u64 *counts;  // [n_values][2]: tp, tp+fn
    u64 *stats;   // [2]: distinct pairs of counting leaves, those found in the store
};

struct GsUpdateParams {
    const u64 *skeys;     // the m stored k-mers, ascending
    int32_t *svals;       // their value indices: updated in place
    int64_t m;
    const void *dir;      // (1 << dir_bits) + 1 bucket starts, uint32_t or (wide) u64
    int32_t dir_bits, wide, k;
    const int32_t *parent, *depth;
    const u64 *keys;      // the slice's pairs
    const uint32_t *region;
    const u64 *n_pairs;   // their number (device: written by the k-mer kernel)
    const int32_t *node_of_region;
    u64 *stats;           // [0] += pairs, [1] += pairs whose k-mer is stored
};

struct GsSizeParams {
    const uint8_t *seq;    // the batch: total bases in n_regions regions, off[n_regions + 1]
    const u64 *off;
    const int32_t *tag;    // value index of each region
    int64_t n_regions, total;
    int32_t k, lower, step, max_dust;
    int32_t hist_shift, hist_bins;  // bin = canonical k-mer >> hist_shift, hist_bins <= 4096
    u64 range_lo, range_hi;         // what is retained (keys != nullptr)
    u64 *totals;           // [3]: total, dust, included
    u64 *per_value;        // per value index
    u64 *hist;             // hist_bins
    u64 *keys;             // nullptr: count only
    u64 *n_keys;           // keys retained so far
    u64 keys_cap;          // room in keys
};

extern "C" {

// ---- gs_kernels.hip: the match kernels and their statistics
hipError_t gs_launch_match(const GsMatchParams *P, int grid, hipStream_t stream);
hipError_t gs_launch_match_huge(const GsMatchParams *P, int grid, hipStream_t stream);
hipError_t gs_launch_match_wide(const GsMatchParams *P, int ns, int n_cu, hipStream_t stream);
int gs_match_wide_mask(const GsMatchParams *P);
hipError_t gs_launch_classify(const GsMatchParams *P, hipStream_t stream);
hipError_t gs_launch_fold_stats(long long *sums, unsigned long long *maxk, double *dsums, long long nv, int copies, unsigned long long *result,
                                hipStream_t stream);
hipError_t gs_launch_match_long(const GsMatchParams *P, int grid, int32_t *scratch, uint32_t *serial, hipStream_t stream);
hipError_t gs_launch_stat_reduce(const GsStatRec *recs, const void *count, int64_t n_max, int n_values, void *sums, void *maxk, void *dsums,
                                 int32_t *vi_scratch, hipStream_t stream);
int gs_match_occupancy(int n_values);

// ---- gs_snreduce.hip: the records of the reads of one tax id (GsSnRec) into the counters, behind gs_launch_match
hipError_t gs_launch_sn_reduce(const GsSnReduceParams *P, hipStream_t stream);

int gs_match_long_occupancy(int n_values);

// ---- gs_route.hip: the DB-partitioned mode
hipError_t gs_launch_encode(const GsEncodeParams *P, int grid, hipStream_t stream);
hipError_t gs_launch_encode_route(const GsEncodeParams *P, const GsRouteParams *R, int grid, hipStream_t stream);
hipError_t gs_launch_unroute_region(const uint32_t *idx, const int32_t *back, int64_t n, int32_t *nodes, hipStream_t stream);
hipError_t gs_launch_route_count(const u64 *keys, int64_t n, int n_parts, u64 *counts, hipStream_t stream);
hipError_t gs_launch_route_scatter(const u64 *keys, int64_t n, int n_parts, u64 *cursors, u64 *send_keys, uint32_t *idx, int32_t *nodes,
                                   hipStream_t stream);
hipError_t gs_launch_unroute(const u64 *keys, const uint32_t *idx, const int32_t *back, int64_t n_routed, int32_t *nodes, int64_t n_keys,
                             hipStream_t stream);
hipError_t gs_launch_probe_keys(const GsDbDev *db, const u64 *keys, int64_t n, int32_t *nodes, int count_unique, hipStream_t stream);

// ---- gs_segments.hip
hipError_t gs_launch_segments(const GsSegParams *P, int write, int grid, hipStream_t stream);

// ---- gs_seen.hip: the seen bits of a store
hipError_t gs_launch_unique_count(const u64 *table, const uint32_t *bitmap, int64_t n_slots, uint32_t vbits, int32_t n_values, u64 *unique,
                                  const u64 *rec, int64_t n_rec, hipStream_t stream);
hipError_t gs_launch_rec_unique_count(const u64 *rec, const uint32_t *bitmap_rec, int64_t n_rec, int32_t n_values, u64 *unique,
                                      hipStream_t stream);
hipError_t gs_launch_clear_seen(u64 *table, int64_t n_slots, u64 *rec, int64_t n_rec, hipStream_t stream);
hipError_t gs_launch_bitmap_extract(const u64 *table, int64_t n_slots, uint32_t *bitmap, const u64 *rec, int64_t n_rec, hipStream_t stream);
hipError_t gs_launch_seen_sweep(const u64 *table, int64_t n_slots, uint32_t vbits, const u64 *rec, int64_t n_rec, uint32_t *bitmap,
                                int32_t n_values, u64 *unique, hipStream_t stream);
hipError_t gs_launch_bitmap_or(uint32_t *dst, const uint32_t *parts, int64_t n_words, int64_t n_parts, hipStream_t stream);

// ---- gs_filter.hip
hipError_t gs_launch_filter(const GsFilterParams *P, int grid, hipStream_t stream);
int gs_filter_occupancy();

// ---- gs_text.hip
hipError_t gs_launch_text_scan(const GsTextParams *P, uint32_t ticket, hipStream_t stream);
hipError_t gs_launch_text_ml(const GsTextParams *P, uint8_t *line_class, hipStream_t stream);
hipError_t gs_launch_text_lines(const GsTextParams *P, hipStream_t stream);
hipError_t gs_launch_text_commit(const GsTextParams *P, uint32_t ticket, hipStream_t stream);

// ---- gs_rewrite.hip: extract and fasta2fastq
hipError_t gs_launch_rewrite_lines(const GsRewriteParams *P, hipStream_t stream);
hipError_t gs_launch_rewrite_heads(const GsRewriteParams *P, hipStream_t stream);
hipError_t gs_launch_rewrite_copy(const GsRewriteParams *P, int64_t out_bound, int n_cu, hipStream_t stream);
hipError_t gs_launch_select(const uint8_t *text, const uint32_t *nl, const uint32_t *rec_line, int64_t n_records, const uint8_t *key, int32_t key_len,
                            const uint32_t *skip, uint8_t *accept, hipStream_t stream);
hipError_t gs_launch_scan_blocks(u64 *blocks, int64_t n_blocks, u64 *total_out, hipStream_t stream);

// ---- gs_kraken.hip: Kraken-style lines as device text
hipError_t gs_launch_kraken_size(const GsKrakenParams *P, hipStream_t stream);
hipError_t gs_launch_kraken_write(const GsKrakenParams *P, hipStream_t stream);

// ---- gs_krakencount.hip: Kraken-style lines counted per tax id
hipError_t gs_launch_krakencount(const GsKrakenCountParams *P, hipStream_t stream);
hipError_t gs_launch_krakencount_reset(const GsKrakenCountParams *P, hipStream_t stream);

// ---- gs_merge.hip: merge of runs that live in one process
hipError_t gs_launch_merge_i64(void *dst, const void *src, int64_t n, int op, hipStream_t stream);
hipError_t gs_launch_merge_f64(void *dst, const void *src, int64_t n, hipStream_t stream);
int gs_rccl_merge_leaders(int n_dev, const int *devices, void *const *sums, void *const *maxk, void *const *dsums, void *const *bitmap,
                          void *const *gather, int64_t n_sums, int64_t n_max, int64_t n_dsums, int64_t n_words, const hipStream_t *streams,
                          const char **msg);

// ---- gs_build.hip
hipError_t gs_launch_build_kmers(const uint8_t *seq, const u64 *off, int64_t n_regions, int64_t total, int k, int lower, int step, int max_dust,
                                 uint32_t first_region, int update, u64 range_lo, u64 range_hi, u64 *keys, uint32_t *vals, u64 *n_out,
                                 hipStream_t stream);
hipError_t gs_build_sort(u64 *keys, u64 *keys_alt, uint32_t *vals, uint32_t *vals_alt, int64_t n, int key_bits, u64 **keys_out,
                         uint32_t **vals_out, hipStream_t stream);
hipError_t gs_build_reduce(const u64 *keys, const uint32_t *vals, int64_t n, const int32_t *node_of_region, const int32_t *parent,
                           const int32_t *depth, uint32_t *flag, int32_t *value, u64 *pos, int64_t *n_out, hipStream_t stream);
hipError_t gs_launch_build_scatter(const u64 *keys, const int32_t *value, const uint32_t *flag, const u64 *pos, int64_t n, int64_t *out_keys,
                                   int32_t *out_vals, hipStream_t stream);
hipError_t gs_launch_bloom_xor_put(const int64_t *keys, int64_t n, int64_t bits, const int64_t *factors, int n_hashes, int murmur, u64 *words,
                                   hipStream_t stream);

// ---- gs_layout_build.hip: the layout built on the device
hipError_t gs_lb_perkey(const int64_t *kmers, const int32_t *vidx, int64_t n, int k, const int32_t *parent, uint32_t *e_gh, uint32_t *e_ohi,
                        uint32_t *e_olo, uint32_t *e_vj, u64 *e_sort, u64 *e_sort2, u64 *t_key, int32_t *t_val, uint32_t *m_gh, uint32_t *h_gh,
                        uint32_t *h_ctx, u64 *cnt, hipStream_t stream);
hipError_t gs_lb_sort_entries(u64 *e_sort, u64 *e_sort2, u64 *sort_alt, uint32_t *perm, uint32_t *perm_alt, int64_t n, const uint32_t *e_gh,
                              const uint32_t *e_ohi, const uint32_t *e_olo, const uint32_t *e_vj, uint32_t *s_gh, uint32_t *s_ohi, uint32_t *s_olo,
                              uint32_t *s_vj, hipStream_t stream);
hipError_t gs_lb_groups(const uint32_t *s_gh, int64_t n, uint32_t *head, uint32_t *group, uint32_t *g_start, int64_t *n_groups,
                        hipStream_t stream);
hipError_t gs_lb_cluster(const uint32_t *s_gh, const uint32_t *s_ohi, const uint32_t *s_olo, const uint32_t *s_vj, const uint32_t *g_start,
                         int64_t n_groups, int k, uint8_t *assign, u64 *w_hi, u64 *w_lo, uint32_t *w_valid, uint32_t *w_gh, u64 *cnt,
                         hipStream_t stream);
hipError_t gs_lb_place(const uint32_t *w_valid, const uint32_t *w_gh, int64_t n_w, uint32_t rec_bits, int max_rounds, uint32_t *slot,
                       uint32_t *slot2, uint32_t *claim, uint32_t *state, uint32_t *win_bucket, u64 *changes, int *rounds_done,
                       hipStream_t stream);
hipError_t gs_lb_lines(const uint32_t *slot, uint32_t rec_bits, const u64 *w_hi, const u64 *w_lo, const uint32_t *w_valid, const uint32_t *s_gh,
                       const uint32_t *s_ohi, const uint32_t *s_olo, const uint32_t *s_vj, const uint32_t *group, const uint8_t *assign,
                       const uint32_t *win_bucket, int64_t n_e, int k, u64 *rec, u64 *t_key, int32_t *t_val, uint32_t *m_gh, u64 *cnt,
                       hipStream_t stream);
hipError_t gs_lb_more(const uint32_t *m_gh, int64_t n_m, uint32_t rec_bits, u64 *rec, hipStream_t stream);
hipError_t gs_lb_table(const u64 *t_key, const int32_t *t_val, int64_t n_t, int b, int vbits, u64 *rot_a, u64 *rot_b, int32_t *val_b,
                       int32_t *val_c, uint32_t *start, uint32_t *left, uint32_t *pos, uint32_t *perm, uint32_t *perm_alt, uint32_t *fill_a,
                       uint32_t *fill_b, u64 *table, int64_t *overflow, int *max_disp, hipStream_t stream);
hipError_t gs_lb_distinct(uint32_t *h_gh, uint32_t *h_alt, int64_t n_h, u64 *d_scratch, int64_t *distinct, uint32_t **sorted,
                          hipStream_t stream);
hipError_t gs_lb_gate(const uint32_t *h_gh, int64_t n_h, int ctx, uint32_t mgate_bits, uint32_t *mgate, hipStream_t stream);
hipError_t gs_lb_hint_collect(const uint32_t *w_valid, const uint32_t *w_gh, const u64 *w_hi, const u64 *w_lo, const uint32_t *win_bucket,
                              int64_t n_w, uint32_t rec_bits, int k, uint32_t *hint_gh, uint32_t *hint_cx, u64 *cnt, hipStream_t stream);
hipError_t gs_lb_hint(const uint32_t *hint_gh, const uint32_t *hint_cx, int64_t n, int ctx, uint32_t mgate_bits, uint32_t *mgate,
                      hipStream_t stream);

// ---- gs_inflate_dev.hip (gs_inflate_last_error: include/gsgpu.h)
int gs_crc_tiles_device(const uint8_t *d_text, int64_t n, uint32_t tile, uint32_t *d_crc, hipStream_t stream);
uint32_t gs_crc_init_term(uint64_t n);

// ---- gs_deflate_dev.hip (gs_deflate_last_error: include/gsgpu.h)
int gs_compact_records_device(hipStream_t stream, const uint8_t *d_text, const uint32_t *d_nl, int64_t n_records, const uint8_t *d_flags,
                              int mask, int want, int with_probs, uint8_t *d_out, uint32_t *d_len, u64 *d_blocks, u64 *h_totals);
int gs_gather_descriptors_device(hipStream_t stream, const uint8_t *d_text, const uint32_t *d_nl, const int64_t *d_records, int n,
                                 uint8_t *d_out, int stride);

// ---- gs_export.hip: the store read back
hipError_t gs_launch_export_decode(const GsExportParams *P, int n_cu, hipStream_t stream);
hipError_t gs_launch_export_fastq(const GsFastqParams *P, void *scratch, size_t *scratch_bytes, int64_t *n_bytes, hipStream_t stream);

// ---- gs_index.hip: the index filter of a store (count pass: P->put == 0; put pass: P->put != 0)
hipError_t gs_launch_index(const GsIndexParams *P, int n_cu, hipStream_t stream);

// ---- gs_prefilter.hip: the 15-mer filter of a store (both levels and |S|), and the reads of a fixed-length batch that pass it
hipError_t gs_launch_prefilter_build(const GsPrefilterBuildParams *P, int n_cu, hipStream_t stream);
hipError_t gs_launch_prefilter(const GsPrefilterParams *P, hipStream_t stream);

// ---- gs_quality.hip
hipError_t gs_launch_quality_tag(uint32_t *vals, int64_t n, const uint32_t *leaf_of_region, int64_t n_regions, hipStream_t stream);
hipError_t gs_quality_sort_leaf(uint32_t *leaf, uint32_t *leaf_alt, u64 *keys, u64 *keys_alt, int64_t n, int bits, uint32_t **leaf_out,
                                u64 **keys_out, hipStream_t stream);
hipError_t gs_launch_quality_join(const GsQualityParams *P, int n_cu, hipStream_t stream);

// ---- gs_update.hip
hipError_t gs_launch_update_check(const u64 *keys, const int32_t *vals, int64_t m, int k, int32_t n_values, uint32_t *flag, int n_cu,
                                  hipStream_t stream);
hipError_t gs_launch_update_dir(const u64 *keys, int64_t m, int k, int dir_bits, int wide, void *dir, int n_cu, hipStream_t stream);
hipError_t gs_launch_update_lookup(const GsUpdateParams *P, int64_t max_pairs, int n_cu, hipStream_t stream);
hipError_t gs_launch_update_moved(const int32_t *vals, const int32_t *vals0, int64_t m, u64 *count, int n_cu, hipStream_t stream);

// ---- gs_genomes.hip: genome FASTA text -> regions
hipError_t gs_launch_genomes_count(const GsGenomesParams *P, hipStream_t stream);
hipError_t gs_launch_genomes_records(const GsGenomesParams *P, hipStream_t stream);
hipError_t gs_launch_genomes_headers(const GsGenomesParams *P, hipStream_t stream);
hipError_t gs_launch_genomes_select(const GsGenomesParams *P, hipStream_t stream);
hipError_t gs_launch_genomes_gather(const GsGenomesParams *P, int64_t cut_tiles, hipStream_t stream);

// ---- gs_size.hip
hipError_t gs_launch_size_count(const GsSizeParams *P, int n_cu, hipStream_t stream);
hipError_t gs_size_sort_bytes(int64_t n, int key_bits, size_t *tmp_bytes);
hipError_t gs_size_sort(u64 *keys, u64 *keys_alt, int64_t n, int key_bits, void *tmp, size_t tmp_bytes, u64 **keys_out, hipStream_t stream);
hipError_t gs_launch_size_heads(const u64 *keys, int64_t n, int radix_bits, u64 *n_distinct, u64 *buckets, int n_cu, hipStream_t stream);

// ---- gs_accmap.hip: RefSeq catalog lines -> accession map
hipError_t gs_launch_accmap_count(const GsAccmapParams *P, hipStream_t stream);
hipError_t gs_launch_accmap_write(const GsAccmapParams *P, hipStream_t stream);
hipError_t gs_accmap_sort_bytes(int64_t n, size_t *tmp_bytes);
// entries [0, n) by key, ties in input order: keys_out / nodes_out / seq_out take them sorted; word / word_alt / seq_alt: n each;
// flag: one word of device memory; counts: [2] adjacent equal keys, those of them with different nodes
hipError_t gs_accmap_sort_entries(const uint8_t *keys, const int32_t *nodes, int64_t n, u64 *word, u64 *word_alt, uint32_t *seq, uint32_t *seq_alt,
                            void *tmp, size_t tmp_bytes, uint32_t *flag, uint8_t *keys_out, int32_t *nodes_out, uint32_t **seq_out, u64 *counts,
                            hipStream_t stream);
hipError_t gs_launch_accmap_lookup(const uint8_t *headers, const u64 *header_off, int64_t n, int complete_only, const uint8_t *keys,
                                   const int32_t *nodes, int64_t n_entries, int32_t *node_out, hipStream_t stream);

// ---- gs_asmsum.hip: assembly summary lines -> per-node picks
// tiles and their scan: scan_tot[0] = newlines | tabs << 32 of the chunk
hipError_t gs_launch_asmsum_tiles(const GsAsmsumParams *P, hipStream_t stream);
// slots of every line, the verdicts, the chunk's counters and the prefix of line_blk: what the write pass would store
hipError_t gs_launch_asmsum_judge(const GsAsmsumParams *P, hipStream_t stream);
// for a chunk that was not refused and whose entries and strings have room
hipError_t gs_launch_asmsum_write(const GsAsmsumParams *P, int64_t n_put, hipStream_t stream);
hipError_t gs_asmsum_cap_bytes(int64_t n, int32_t n_nodes, size_t *tmp_bytes);
// the cap: node_words: 4 * (n_nodes + 1) words (entries per node, their prefix, picks per node, their prefix); key / key_alt / seq /
// seq_alt / perm: n each; counts: [2] picked entries, nodes with entries.  perm[0 .. picked) are the entry numbers, nodes ascending,
// inside a node the reference's list order
hipError_t gs_asmsum_cap(const GsAsmEntry *entries, int64_t n, int32_t n_nodes, int32_t max_per_node, uint32_t *node_words, u64 *key, u64 *key_alt,
                         uint32_t *seq, uint32_t *seq_alt, void *tmp, size_t tmp_bytes, uint32_t *perm, u64 *counts, hipStream_t stream);
// lens: 3 m + 1 words of scratch; str_off: 3 m + 1 offsets into pool_out, which takes the strings; out[j] = entries[perm[j]] with
// pool_off = str_off[3 j]
hipError_t gs_asmsum_pick_sizes(const GsAsmEntry *entries, const uint32_t *perm, int64_t m, u64 *lens, u64 *str_off, void *tmp, size_t tmp_bytes,
                                hipStream_t stream);
hipError_t gs_asmsum_pick_gather(const GsAsmEntry *entries, const uint32_t *perm, int64_t m, const u64 *str_off, const uint8_t *pool, GsAsmEntry *out,
                                 uint8_t *pool_out, hipStream_t stream);

// ---- gs_taxtree.hip: nodes.dmp lines -> tree arrays; select; small tree
hipError_t gs_launch_taxtree_tiles(const GsTaxScanParams *P, hipStream_t stream);
hipError_t gs_launch_taxtree_scan(const GsTaxScanParams *P, hipStream_t stream);
hipError_t gs_launch_taxtree_names(const GsTaxScanParams *P, int mode, hipStream_t stream);
hipError_t gs_taxtree_sort_bytes(int64_t n_keys, size_t *tmp_bytes);
hipError_t gs_taxtree_distinct(const uint4 *slots, int64_t m, uint32_t *keys, uint32_t *keys_alt, uint32_t *head, uint32_t *idx, void *tmp, size_t tmp_bytes,
                               int32_t *taxids, u64 *counts, hipStream_t stream);
hipError_t gs_taxtree_resolve(const uint4 *slots, int64_t m, const GsTaxTreeArrays *A, u64 *counts, hipStream_t stream);
hipError_t gs_taxtree_children(const GsTaxTreeArrays *A, u64 *key, u64 *key_alt, uint32_t *ord, uint32_t *ord_alt, void *tmp, size_t tmp_bytes,
                               int32_t *first_child, int32_t *next_sib, hipStream_t stream);
hipError_t gs_taxtree_place(const GsTaxTreeArrays *A, const int32_t *first_child, const int32_t *next_sib, uint32_t *succ, uint32_t *succ_alt, u64 *val,
                            u64 *val_alt, int32_t *up, int32_t *up_alt, u64 *counts, hipStream_t stream);
hipError_t gs_launch_taxtree_select(const GsTaxTreeArrays *A, const int32_t *requested, int64_t n_req, const int32_t *excluded, int64_t n_exc, int cut,
                                    uint8_t *marks, int32_t *anc, uint8_t *out, u64 *count, hipStream_t stream);
hipError_t gs_launch_taxtree_small(const GsTaxTreeArrays *A, int32_t n_reach, const uint8_t *flag8, const int32_t *flag32, uint32_t *pre, uint32_t *sum,
                                   uint32_t *req, uint32_t *vi, void *tmp, size_t tmp_bytes, int32_t *node_of_vi, int32_t *parent_vi, int32_t *depth,
                                   int32_t *position, hipStream_t stream);
hipError_t gs_launch_taxtree_regions(const GsTaxTreeArrays *A, int32_t n_reach, const int32_t *regions, uint32_t *pre, uint32_t *sum, void *tmp, size_t tmp_bytes,
                                     int32_t *incl, hipStream_t stream);
hipError_t gs_launch_taxtree_below(const GsTaxTreeArrays *A, const int32_t *selected, int64_t n_sel, const int32_t *incl, int32_t limit, int check_rank,
                                   uint8_t *marks, uint32_t *flag, uint32_t *idx, void *tmp, size_t tmp_bytes, int32_t *out, hipStream_t stream);

}  // extern "C"

// ---- gs_devcache.cpp: the device block cache.  Every device allocation of gs_api.cpp goes through these two, by name; hidden,
// so that the library exports neither.
__attribute__((visibility("hidden"))) hipError_t gs_dev_alloc(void **p, size_t n);
__attribute__((visibility("hidden"))) hipError_t gs_dev_free(void *p);
template <typename T>
static inline hipError_t gs_dev_alloc(T **p, size_t n) {
    return gs_dev_alloc(reinterpret_cast<void **>(p), n);
}
