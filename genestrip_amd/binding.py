"""ctypes binding of include/gsgpu.h (libgsgpu.so).

Host-side mirror of the reference interface for the hot path:

* ``DeviceKMerStore``   <- KMerStore + SmallTaxTree as the matcher sees them (C/store/KMerStore.java:45-317)
* ``FastqKMerMatcher``  <- C/match/FastqKMerMatcher.java (runMatcher :181-235, matchRead :327-535)
* ``DeviceBloomFilter`` <- KMerProbFilter (C/bloom/AbstractKMerBloomFilter.java, BlockedKMerBloomFilter.java)
* ``FastqBloomFilter``  <- C/bloom/FastqBloomFilter.java (runFilter :80-89, isAcceptRead :120-161)

numpy arrays are host batches (GS_MEM_HOST); objects exposing ``data_ptr()`` (torch tensors on the GPU) are
passed as device batches (GS_MEM_DEVICE).
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

N_COLS, N_DCOLS, N_SUMS = 10, 4, 7
COLS = ("reads", "kmers from reads", "kmers", "unique kmers", "contigs", "contig len sq sum", "max contig length",
        "reads >=1 kmer", "reads bps", "max contig read no")
MEM_HOST, MEM_DEVICE = 0, 1
F_FOUND, F_RETURNED, F_COUNTED = 1, 2, 4
BLOOM_XOR, BLOOM_MURMUR, BLOOM_BLOCKED = 0, 1, 2

# every symbol include/gsgpu.h declares (checked by the CPU test-suite against the built library)
ABI_SYMBOLS = (
    "gs_last_error", "gs_strerror", "gs_device_cache_trim", "gs_abi_version", "gs_device_count",
    "gs_match_merge", "gs_match_max_contig_reads", "gs_db_create", "gs_db_get_info", "gs_db_destroy", "gs_db_save", "gs_db_load",
    "gs_match_begin", "gs_match_submit", "gs_match_submit_async", "gs_match_wait", "gs_match_sync", "gs_match_finish", "gs_match_reset", "gs_match_destroy",
    "gs_match_device_state", "gs_match_or_bitmap", "gs_match_kernel_time", "gs_match_prefilter_info", "gs_match_sn_info", "gs_match_gate_info", "gs_match_gate_rule", "gs_match_segments",
    "gs_match_segments_fetch", "gs_match_max_counts", "gs_db_create_striped", "gs_db_create_stripe", "gs_db_stripe_export", "gs_db_stripe_attach", "gs_db_load_striped", "gs_db_load_stripe", "gs_dbbuild_begin", "gs_dbbuild_set_range", "gs_dbbuild_add", "gs_dbbuild_finish", "gs_dbbuild_fetch", "gs_dbbuild_to_db", "gs_dbbuild_destroy", "gs_db_create_part", "gs_match_encode", "gs_match_probe_keys", "gs_match_encode_route", "gs_match_route_geometry", "gs_unroute_region", "gs_match_reduce", "gs_route_keys",
    "gs_unroute_nodes",
    "gs_match_submit_text", "gs_match_submit_fasta", "gs_match_submit_fastq_ml", "gs_match_text_wait_copy", "gs_match_text_status", "gs_match_text_clear_error",
    "gs_match_text_select", "gs_match_segments_text", "gs_match_text_newlines", "gs_match_text_read_bounds", "gs_match_text_line_classes",
    "gs_pinned_alloc", "gs_pinned_free",
    "gs_filter_submit_text", "gs_filter_text_wait_copy", "gs_filter_text_status", "gs_filter_text_reset",
    "gs_filter_submit_fasta", "gs_filter_submit_fastq_ml", "gs_filter_text_read_bounds", "gs_filter_text_line_classes",
    "gs_bloom_create", "gs_bloom_build", "gs_bloom_get", "gs_bloom_destroy",
    "gs_bloom_build_db", "gs_bloom_get_info", "gs_bloom_save", "gs_bloom_load", "gs_filter_submit", "gs_filter_sync", "gs_filter_kernel_time",
    "gs_calibrate",
    "gs_match_get_device", "gs_inflate_members", "gs_inflater_create", "gs_inflater_feed", "gs_inflater_tail", "gs_gunzipper_open", "gs_gunzipper_reopen", "gs_gunzipper_next", "gs_gunzipper_info", "gs_gunzipper_first_span", "gs_gunzipper_park", "gs_gunzipper_close", "gs_gunzip_plan_device", "gs_gunzip_free", "gs_gunzip_device", "gs_text_cut_device", "gs_device_fetch", "gs_inflater_fetch", "gs_filter_get_device", "gs_inflater_reset", "gs_inflater_destroy", "gs_inflate_last_error",
    "gs_filter_compact_text", "gs_match_compact_text", "gs_filter_compact_records", "gs_match_compact_records", "gs_match_kraken_records", "gs_match_set_taxids", "gs_match_kraken_text", "gs_match_kraken_time", "gs_deflater_create", "gs_deflater_pack", "gs_deflater_info", "gs_deflater_destroy", "gs_deflater_append", "gs_deflater_pending", "gs_deflater_flush",
    "gs_deflate_bound", "gs_deflate_host", "gs_deflate_host_reference", "gs_deflate_last_error", "gs_match_text_descriptors", "gs_match_submit_fixed",
    "gs_db_value_counts", "gs_dbexport_create", "gs_dbexport_fetch", "gs_dbexport_get_device", "gs_dbexport_fastq_begin",
    "gs_dbexport_fastq_next", "gs_dbexport_destroy",
    "gs_dbquality_begin", "gs_dbquality_set_range", "gs_dbquality_add", "gs_dbquality_finish", "gs_dbquality_get_stats",
    "gs_dbquality_destroy",
    "gs_dbupdate_begin", "gs_dbupdate_begin_db", "gs_dbupdate_begin_build", "gs_dbupdate_set_slice", "gs_dbupdate_add",
    "gs_dbupdate_finish", "gs_dbupdate_fetch", "gs_dbupdate_to_db", "gs_dbupdate_get_stats", "gs_dbupdate_destroy",
    "gs_dbsize_begin", "gs_dbsize_set_range", "gs_dbsize_add", "gs_dbsize_counts", "gs_dbsize_distinct", "gs_dbsize_get_stats",
    "gs_dbsize_destroy", "gs_dbsize_plan",
    "gs_reads_create", "gs_reads_destroy", "gs_reads_get_device", "gs_reads_sync", "gs_reads_select_text", "gs_reads_select_fasta",
    "gs_reads_select_fastq_ml", "gs_reads_compact_text", "gs_reads_compact_records", "gs_reads_fasta2fastq", "gs_reads_text_read_bounds", "gs_reads_text_line_classes",
    "gs_reads_text_wait_copy", "gs_reads_text_status", "gs_reads_text_reset", "gs_reads_kernel_time",
    "gs_reads_phase_times",
    "gs_krakencount_create", "gs_krakencount_destroy", "gs_krakencount_get_device", "gs_krakencount_geometry", "gs_krakencount_submit",
    "gs_krakencount_chunk", "gs_krakencount_status", "gs_krakencount_reset", "gs_krakencount_fetch", "gs_krakencount_counters",
    "gs_krakencount_kernel_time",
    "gs_genomes_create", "gs_genomes_scan", "gs_genomes_headers", "gs_genomes_gather", "gs_genomes_regions", "gs_genomes_kernel_time",
    "gs_genomes_destroy",
    "gs_accmap_create", "gs_accmap_submit", "gs_accmap_append", "gs_accmap_finish", "gs_accmap_fetch", "gs_accmap_lookup",
    "gs_accmap_lookup_genomes", "gs_accmap_get_device", "gs_accmap_get_n_nodes", "gs_accmap_kernel_time", "gs_accmap_destroy",
    "gs_asmsum_create", "gs_asmsum_submit", "gs_asmsum_append", "gs_asmsum_finish", "gs_asmsum_fetch", "gs_asmsum_file_name",
    "gs_asmsum_get_device", "gs_asmsum_kernel_time", "gs_asmsum_destroy",
    "gs_taxtree_create", "gs_taxtree_submit_nodes", "gs_taxtree_append_nodes", "gs_taxtree_finish_nodes", "gs_taxtree_submit_names", "gs_taxtree_append_names", "gs_taxtree_finish_times",
    "gs_taxtree_fetch", "gs_taxtree_fetch_names", "gs_taxtree_select", "gs_taxtree_small", "gs_taxtree_regions_below", "gs_taxtree_read_taxids",
    "gs_taxtree_get_device", "gs_taxtree_kernel_time", "gs_taxtree_destroy",
)


class GsError(RuntimeError):
    """non-zero status from the C ABI (the JNI shim turns the same codes into RuntimeException)"""

    def __init__(self, code, msg):
        super().__init__(f"gsgpu error {code}: {msg}")
        self.code = code


class DbInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("n_values", C.c_int32), ("n_entries", C.c_int64), ("n_stored", C.c_int64),
                ("n_buckets", C.c_int64), ("table_bytes", C.c_int64), ("max_displacement", C.c_int32),
                ("value_bits", C.c_int32), ("gate_bytes", C.c_int64), ("mgate_bytes", C.c_int64),
                ("rec_bytes", C.c_int64), ("n_in_records", C.c_int64), ("n_stripes", C.c_int32), ("stripe", C.c_int32),
                ("stripe_bytes", C.c_int64)]


class _MatchCfg(C.Structure):
    _fields_ = [("classify", C.c_int32), ("count_unique", C.c_int32), ("max_paths", C.c_int32),
                ("threshold", C.c_int32), ("max_read_tax_err", C.c_double), ("max_read_class_err", C.c_double),
                ("profile", C.c_int32), ("max_kmer_res_counts", C.c_int32)]


def lib_path():
    # GS_LIBGSGPU: developer override used to A/B kernel build variants on the GPU box
    return os.environ.get("GS_LIBGSGPU") or os.path.join(_HERE, "libgsgpu.so")


def _preload_hip_runtime():
    """One HIP runtime per process.  libgsgpu.so needs `libamdhip64.so.7`; a PyTorch-ROCm wheel ships its own
    copy (same SONAME) next to libtorch_hip.so.  Whichever copy is loaded first serves both, so when torch is
    installed its copy is loaded first -- then torch (device memory, torch.distributed/RCCL in bench.py and
    the tests) and this library share a single runtime and a single set of device contexts.  Set
    GS_HIP_RUNTIME=system to skip this (e.g. under a JVM without torch)."""
    if os.environ.get("GS_HIP_RUNTIME", "") == "system":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """load libgsgpu.so; raises if it was not built (no fallback implementation exists)"""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise GsError(-6, f"{path} is missing: build it with `make -C genestrip_amd/csrc` (hipcc, gfx950); "
                          "genestrip_amd has no CPU fallback")
    _preload_hip_runtime()
    L = C.CDLL(path)
    vp, i32, i64, dbl, ci = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_int
    sig = {
        "gs_last_error": (C.c_char_p, []), "gs_strerror": (C.c_char_p, [ci]), "gs_device_cache_trim": (ci, []), "gs_abi_version": (ci, []),
        "gs_device_count": (ci, [vp]),
        "gs_db_create": (ci, [vp, ci, ci, i64, vp, vp, i32, vp]), "gs_db_get_info": (ci, [vp, vp]),
        "gs_db_destroy": (ci, [vp]), "gs_db_save": (ci, [vp, C.c_char_p]), "gs_db_load": (ci, [vp, ci, C.c_char_p]),
        "gs_match_begin": (ci, [vp, vp, vp]), "gs_match_submit": (ci, [vp, vp, vp, i64, i64, ci, vp, vp]),
        "gs_match_submit_async": (ci, [vp, vp, vp, i64, i64, vp, vp, vp]), "gs_match_wait": (ci, [vp, i64]),
        "gs_match_sync": (ci, [vp]), "gs_match_finish": (ci, [vp, vp, vp]), "gs_match_reset": (ci, [vp]),
        "gs_match_destroy": (ci, [vp]), "gs_match_device_state": (ci, [vp, vp, vp, vp, vp, vp]),
        "gs_match_or_bitmap": (ci, [vp, vp, i64]), "gs_match_merge": (ci, [vp, ci]), "gs_match_max_contig_reads": (ci, [vp, vp]), "gs_match_kernel_time": (ci, [vp, vp, vp]), "gs_match_prefilter_info": (ci, [vp, vp]), "gs_match_sn_info": (ci, [vp, vp]),
        "gs_match_gate_info": (ci, [vp, vp, vp]), "gs_match_gate_rule": (ci, [i64, ci, ci, vp]),
        "gs_db_create_part": (ci, [vp, ci, ci, i64, vp, vp, i32, vp, ci, ci]),
        "gs_db_create_striped": (ci, [vp, vp, ci, ci, i64, vp, vp, i32, vp]),
        "gs_db_create_stripe": (ci, [vp, ci, ci, ci, ci, i64, vp, vp, i32, vp]),
        "gs_db_stripe_export": (ci, [vp, vp]),
        "gs_db_stripe_attach": (ci, [vp, ci, vp]),
        "gs_db_load_striped": (ci, [vp, vp, ci, C.c_char_p]),
        "gs_db_load_stripe": (ci, [vp, ci, ci, ci, C.c_char_p]),
        "gs_dbbuild_begin": (ci, [vp, ci, ci, i32, vp, ci, ci, ci]),
        "gs_dbbuild_add": (ci, [vp, vp, vp, vp, i64, ci, ci]),
        "gs_dbbuild_set_range": (ci, [vp, C.c_uint64, C.c_uint64]),
        "gs_dbbuild_finish": (ci, [vp, vp]),
        "gs_dbbuild_fetch": (ci, [vp, vp, vp]),
        "gs_dbbuild_to_db": (ci, [vp, vp]),
        "gs_dbbuild_destroy": (ci, [vp]),
        "gs_dbquality_begin": (ci, [vp, vp, ci, ci, ci]),
        "gs_dbquality_set_range": (ci, [vp, C.c_uint64, C.c_uint64]),
        "gs_dbquality_add": (ci, [vp, vp, vp, vp, i64, ci]),
        "gs_dbquality_finish": (ci, [vp, vp, vp]),
        "gs_dbquality_get_stats": (ci, [vp, vp]),
        "gs_dbquality_destroy": (ci, [vp]),
        "gs_dbupdate_begin": (ci, [vp, ci, ci, i32, vp, ci, ci, ci, vp, vp, i64, ci]),
        "gs_dbupdate_begin_db": (ci, [vp, vp, ci, ci, ci]),
        "gs_dbupdate_begin_build": (ci, [vp, vp]),
        "gs_dbupdate_set_slice": (ci, [vp, i64]),
        "gs_dbupdate_add": (ci, [vp, vp, vp, vp, i64, ci]),
        "gs_dbupdate_finish": (ci, [vp, vp]),
        "gs_dbupdate_fetch": (ci, [vp, vp, vp]),
        "gs_dbupdate_to_db": (ci, [vp, vp]),
        "gs_dbupdate_get_stats": (ci, [vp, vp]),
        "gs_dbupdate_destroy": (ci, [vp]),
        "gs_dbsize_begin": (ci, [vp, ci, ci, i32, ci, ci, ci, ci, ci, ci]),
        "gs_dbsize_set_range": (ci, [vp, C.c_uint64, C.c_uint64]),
        "gs_dbsize_add": (ci, [vp, vp, vp, vp, i64, ci]),
        "gs_dbsize_counts": (ci, [vp, vp, vp, vp]),
        "gs_dbsize_distinct": (ci, [vp, vp, vp]),
        "gs_dbsize_get_stats": (ci, [vp, vp]),
        "gs_dbsize_destroy": (ci, [vp]),
        "gs_dbsize_plan": (ci, [vp, ci, ci, i64, vp, ci, vp]),
        "gs_match_encode": (ci, [vp, vp, vp, i64, vp, vp]), "gs_match_probe_keys": (ci, [vp, vp, i64, vp]),
        "gs_match_encode_route": (ci, [vp, vp, vp, i64, vp, ci, i64, vp, vp, vp, vp, vp]),
        "gs_match_route_geometry": (ci, [vp, i64, vp, vp]),
        "gs_unroute_region": (ci, [vp, vp, vp, i64, vp]),
        "gs_match_reduce": (ci, [vp, vp, vp, i64, i64, vp, vp, vp, vp]),
        "gs_route_keys": (ci, [vp, vp, i64, ci, vp, vp, vp, vp]), "gs_unroute_nodes": (ci, [vp, vp, vp, vp, i64, vp, i64]),
        "gs_match_max_counts": (ci, [vp, vp]),
        "gs_match_submit_text": (ci, [vp, vp, i64, i64, ci, i64, vp, vp, vp]),
        "gs_match_submit_fasta": (ci, [vp, vp, i64, i64, i64, ci, i64, vp, vp, vp]),
        "gs_match_submit_fastq_ml": (ci, [vp, vp, i64, i64, ci, i64, vp, vp, vp, vp, vp, vp]),
        "gs_match_text_line_classes": (ci, [vp, vp]),
        "gs_match_text_wait_copy": (ci, [vp, i64]), "gs_match_text_status": (ci, [vp, vp, vp, vp]),
        "gs_match_text_clear_error": (ci, [vp]), "gs_match_text_select": (ci, [vp, ci]),
        "gs_match_segments_text": (ci, [vp, vp]), "gs_match_text_newlines": (ci, [vp, vp]),
        "gs_match_text_read_bounds": (ci, [vp, vp]),
        "gs_pinned_alloc": (ci, [vp, C.c_size_t]), "gs_pinned_free": (ci, [vp]),
        "gs_filter_submit_text": (ci, [vp, ci, ci, dbl, vp, i64, i64, ci, vp, vp, ci, vp]),
        "gs_filter_text_wait_copy": (ci, [vp, i64]), "gs_filter_text_status": (ci, [vp, vp, vp, vp]),
        "gs_filter_text_reset": (ci, [vp, ci]),
        "gs_filter_submit_fasta": (ci, [vp, ci, ci, dbl, vp, i64, i64, i64, ci, vp, vp, vp]),
        "gs_filter_submit_fastq_ml": (ci, [vp, ci, ci, dbl, vp, i64, i64, ci, vp, vp, vp, vp, vp, vp]),
        "gs_filter_text_read_bounds": (ci, [vp, vp]), "gs_filter_text_line_classes": (ci, [vp, vp]),
        "gs_match_segments": (ci, [vp, vp, vp, i64, ci, vp]), "gs_match_segments_fetch": (ci, [vp, vp, vp]),
        "gs_bloom_create": (ci, [vp, ci, ci, i64, i32, vp, vp, i64]),
        "gs_bloom_build": (ci, [vp, ci, ci, vp, i64, ci, i64, C.c_double]),
        "gs_bloom_get": (ci, [vp, vp, vp, vp, vp, i64]), "gs_bloom_destroy": (ci, [vp]),
        "gs_bloom_build_db": (ci, [vp, vp, ci, vp, i64, C.c_double, vp]), "gs_bloom_get_info": (ci, [vp, vp]),
        "gs_bloom_save": (ci, [vp, C.c_char_p]), "gs_bloom_load": (ci, [vp, ci, C.c_char_p]),
        "gs_filter_submit": (ci, [vp, ci, ci, dbl, vp, vp, i64, ci, vp, ci]), "gs_filter_sync": (ci, [vp]),
        "gs_filter_kernel_time": (ci, [vp, vp, vp]),
        "gs_calibrate": (ci, [ci, ci, i64, vp]),
        "gs_match_get_device": (ci, [vp, vp]),
        "gs_inflate_members": (ci, [ci, vp, vp, i64, vp, i64, vp]),
        "gs_inflater_create": (ci, [vp, ci]),
        "gs_inflater_feed": (ci, [vp, vp, vp, i64, i64, i64, ci, vp, vp, vp, vp]),
        "gs_inflater_tail": (ci, [vp, vp, i64, vp]),
        "gs_inflater_fetch": (ci, [vp, vp, i64]),
        "gs_gunzipper_open": (ci, [vp, ci, vp, i64]),
        "gs_gunzipper_reopen": (ci, [vp, vp, i64]),
        "gs_gunzipper_next": (ci, [vp, i64, vp, vp, vp]),
        "gs_gunzipper_info": (ci, [vp, vp]),
        "gs_gunzipper_first_span": (ci, [vp, i64]),
        "gs_gunzipper_park": (ci, [vp]),
        "gs_gunzipper_close": (ci, [vp]),
        "gs_gunzip_plan_device": (ci, [ci, vp, i64, vp, vp, vp]),
        "gs_gunzip_free": (ci, [ci, vp]),
        "gs_gunzip_device": (ci, [ci, vp, i64, vp, i64, vp, vp]),
        "gs_text_cut_device": (ci, [ci, vp, i64, vp, vp]),
        "gs_device_fetch": (ci, [ci, vp, vp, i64]),
        "gs_filter_get_device": (ci, [vp, vp]),
        "gs_inflater_reset": (ci, [vp]),
        "gs_inflater_destroy": (ci, [vp]),
        "gs_inflate_last_error": (C.c_char_p, []),
        "gs_filter_compact_text": (ci, [vp, ci, ci, ci, vp, vp, vp]),
        "gs_match_compact_text": (ci, [vp, ci, ci, vp, vp, vp]),
        "gs_filter_compact_records": (ci, [vp, ci, ci, ci, vp, vp, vp]),
        "gs_match_compact_records": (ci, [vp, ci, ci, vp, vp, vp]),
        "gs_match_kraken_records": (ci, [vp, ci, ci, vp, vp, vp]),
        "gs_match_set_taxids": (ci, [vp, vp]), "gs_match_kraken_text": (ci, [vp, ci, ci, vp, vp, vp]),
        "gs_match_kraken_time": (ci, [vp, vp, vp]),
        "gs_deflater_create": (ci, [vp, ci]),
        "gs_deflater_pack": (ci, [vp, vp, i64, vp, i64, vp]),
        "gs_deflater_info": (ci, [vp, vp]),
        "gs_deflater_append": (ci, [vp, vp, i64]),
        "gs_deflater_pending": (i64, [vp]),
        "gs_deflater_flush": (ci, [vp, vp, i64, vp]),
        "gs_deflater_destroy": (ci, [vp]),
        "gs_deflate_bound": (i64, [i64]),
        "gs_deflate_host": (ci, [ci, vp, i64, vp, i64, vp]),
        "gs_deflate_host_reference": (ci, [vp, i64, vp, i64, vp]),
        "gs_deflate_last_error": (C.c_char_p, []),
        "gs_match_text_descriptors": (ci, [vp, vp, i32, vp, i32]),
        "gs_match_submit_fixed": (ci, [vp, vp, i32, i64, i64, ci, vp, vp]),
        "gs_db_value_counts": (ci, [vp, vp]),
        "gs_dbexport_create": (ci, [vp, vp, i32, ci, vp]),
        "gs_dbexport_fetch": (ci, [vp, vp, vp, ci]),
        "gs_dbexport_get_device": (ci, [vp, vp]),
        "gs_dbexport_fastq_begin": (ci, [vp, vp, C.c_char_p]),
        "gs_dbexport_fastq_next": (ci, [vp, vp, vp, vp]),
        "gs_dbexport_destroy": (ci, [vp]),
        "gs_reads_create": (ci, [vp, ci]), "gs_reads_destroy": (ci, [vp]), "gs_reads_get_device": (ci, [vp, vp]), "gs_reads_sync": (ci, [vp]),
        "gs_reads_select_text": (ci, [vp, ci, vp, i64, i64, ci, vp, i32, vp, vp, vp]),
        "gs_reads_select_fasta": (ci, [vp, ci, vp, i64, i64, i64, ci, vp, i32, vp, vp, vp]),
        "gs_reads_select_fastq_ml": (ci, [vp, ci, vp, i64, i64, ci, vp, i32, vp, vp, vp, vp, vp, vp]),
        "gs_reads_compact_text": (ci, [vp, ci, ci, vp, vp, vp]),
        "gs_reads_compact_records": (ci, [vp, ci, ci, vp, vp, vp]),
        "gs_reads_fasta2fastq": (ci, [vp, vp, i64, i64, i64, ci, ci, vp, vp, vp, vp]),
        "gs_reads_text_read_bounds": (ci, [vp, vp]), "gs_reads_text_line_classes": (ci, [vp, vp]),
        "gs_reads_text_wait_copy": (ci, [vp, i64]), "gs_reads_text_status": (ci, [vp, vp, vp, vp]), "gs_reads_text_reset": (ci, [vp, ci]),
        "gs_reads_kernel_time": (ci, [vp, ci, vp, vp]), "gs_reads_phase_times": (ci, [vp, vp, vp]),
        "gs_krakencount_create": (ci, [vp, ci, i64]), "gs_krakencount_destroy": (ci, [vp]), "gs_krakencount_get_device": (ci, [vp, vp]),
        "gs_krakencount_geometry": (ci, [vp, vp]), "gs_krakencount_submit": (ci, [vp, vp, i64, ci, vp]),
        "gs_krakencount_chunk": (ci, [vp, i64, vp]), "gs_krakencount_status": (ci, [vp, vp, vp, vp, vp]), "gs_krakencount_reset": (ci, [vp]),
        "gs_krakencount_fetch": (ci, [vp, vp, vp, i64, vp]), "gs_krakencount_counters": (ci, [vp, vp]),
        "gs_krakencount_kernel_time": (ci, [vp, ci, vp, vp]),
        "gs_accmap_create": (ci, [vp, ci, vp]), "gs_accmap_submit": (ci, [vp, vp, i64, ci, ci, vp]),
        "gs_accmap_append": (ci, [vp, vp, vp, i64, i64]), "gs_accmap_finish": (ci, [vp, vp]), "gs_accmap_fetch": (ci, [vp, vp, vp, vp]),
        "gs_accmap_lookup": (ci, [vp, vp, vp, i64, ci, ci, vp]), "gs_accmap_lookup_genomes": (ci, [vp, vp, ci, vp]),
        "gs_accmap_get_device": (ci, [vp, vp]), "gs_accmap_get_n_nodes": (ci, [vp, vp]), "gs_accmap_kernel_time": (ci, [vp, ci, vp, vp]), "gs_accmap_destroy": (ci, [vp]),
        "gs_asmsum_create": (ci, [vp, ci, vp]), "gs_asmsum_submit": (ci, [vp, vp, i64, ci, ci, vp]),
        "gs_asmsum_append": (ci, [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64]), "gs_asmsum_finish": (ci, [vp, i32, vp]),
        "gs_asmsum_fetch": (ci, [vp, vp, vp, vp, vp, vp, vp]), "gs_asmsum_file_name": (i64, [C.c_char_p, i64, vp, i64]),
        "gs_asmsum_get_device": (ci, [vp, vp]), "gs_asmsum_kernel_time": (ci, [vp, ci, vp, vp]), "gs_asmsum_destroy": (ci, [vp]),
        "gs_taxtree_create": (ci, [vp, ci]), "gs_taxtree_submit_nodes": (ci, [vp, vp, i64, ci, ci, vp]),
        "gs_taxtree_append_nodes": (ci, [vp, vp, i64, ci, vp]), "gs_taxtree_finish_nodes": (ci, [vp, vp]),
        "gs_taxtree_append_names": (ci, [vp, vp, i64, ci]), "gs_taxtree_submit_names": (ci, [vp, vp, i64, ci, ci, vp]),
        "gs_taxtree_finish_times": (ci, [vp, vp]), "gs_taxtree_fetch": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "gs_taxtree_fetch_names": (ci, [vp, vp, vp, i64]), "gs_taxtree_select": (ci, [vp, vp, i64, vp, i64, ci, vp, vp]),
        "gs_taxtree_small": (ci, [vp, vp, ci, ci, vp, vp, vp, vp, vp]), "gs_taxtree_read_taxids": (ci, [vp, i64, vp, vp, vp, vp, i64]),
        "gs_taxtree_regions_below": (ci, [vp, vp, ci, vp, i64, i32, ci, vp, vp, vp]),
        "gs_taxtree_get_device": (ci, [vp, vp]), "gs_taxtree_kernel_time": (ci, [vp, ci, vp, vp]), "gs_taxtree_destroy": (ci, [vp]),
        "gs_genomes_create": (ci, [vp, ci]), "gs_genomes_scan": (ci, [vp, vp, i64, ci, ci, vp, vp, vp, vp]),
        "gs_genomes_headers": (ci, [vp, vp, vp]), "gs_genomes_gather": (ci, [vp, vp, vp, vp]), "gs_genomes_regions": (ci, [vp, vp, vp]),
        "gs_genomes_kernel_time": (ci, [vp, vp, vp]), "gs_genomes_destroy": (ci, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    _LIB = L
    return L


def _check(rc):
    if rc != 0:
        raise GsError(rc, (lib().gs_last_error() or b"").decode(errors="replace"))


def abi_version():
    return lib().gs_abi_version()


def device_count():
    n = C.c_int(0)
    rc = lib().gs_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def gate_rule(n_lmers, samples, mode=-1):
    """The rule by which a prefiltered fixed-length batch drops the minimizer gate (gs_match_gate_rule, a pure function):
    (gateless, predicted_pass) for a store of n_lmers distinct canonical 15-mers and `samples` sampled 15-mers per read;
    mode is the value of GS_PF_GATE, -1 when unset."""
    p = C.c_double(0)
    g = lib().gs_match_gate_rule(int(n_lmers), int(samples), int(mode), C.byref(p))
    return bool(g), p.value


class InflateMember(C.Structure):
    _fields_ = [("payload_offset", C.c_int64), ("payload_len", C.c_uint32), ("isize", C.c_uint32), ("crc32", C.c_uint32),
                ("reserved", C.c_uint32)]


def bgzf_members(data):
    """the members of a BGZF buffer (bytes / numpy uint8), found from their headers alone: list of (payload_offset,
    payload_len, isize, crc32); stops at the first thing that is not a BGZF member -> (members, offset reached)"""
    import struct
    b = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
    out, o, n = [], 0, len(b)
    while o + 28 <= n and b[o] == 0x1f and b[o + 1] == 0x8b and b[o + 2] == 8 and (b[o + 3] & 4):
        if b[o + 3] & ~4:  # name / comment / header CRC: not what bgzip writes
            break
        xlen = struct.unpack_from("<H", b, o + 10)[0]
        q, bsize = o + 12, None
        while q + 4 <= o + 12 + xlen:
            slen = struct.unpack_from("<H", b, q + 2)[0]
            if b[q:q + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", b, q + 4)[0]
            q += 4 + slen
        if bsize is None or o + bsize + 1 > n or bsize + 1 < 12 + xlen + 8:
            break
        end = o + bsize + 1
        crc, isize = struct.unpack_from("<II", b, end - 8)
        if isize > 65536:
            break
        out.append((o + 12 + xlen, end - 8 - (o + 12 + xlen), isize, crc))
        o = end
    return out, o


def inflate_members(data, members, device=0):
    """gs_inflate_members: -> (text bytes as numpy uint8, status int32[]); raises GsError when a member is corrupt"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    arr = (InflateMember * max(1, len(members)))()
    total = 0
    for i, (po, pl, isz, crc) in enumerate(members):
        arr[i] = InflateMember(po, pl, isz, crc, 0)
        total += isz
    out = np.zeros(max(total, 1), dtype=np.uint8)
    st = np.full(max(len(members), 1), -1, dtype=np.int32)
    rc = lib().gs_inflate_members(device, buf.ctypes.data_as(C.c_void_p), arr, len(members), out.ctypes.data_as(C.c_void_p), total,
                                  st.ctypes.data_as(C.c_void_p))
    if rc != 0:
        e = GsError(rc, (lib().gs_inflate_last_error() or b"").decode(errors="replace"))
        e.status = st[:len(members)].copy()
        raise e
    return out[:total], st[:len(members)]


def gunzip_device(data, expect_bytes, device=0):
    """gs_gunzip_device: a single-member gzip stream inflated on the device -> (text as numpy uint8, info[4] = segments, chunks searched,
    batches, mirages); raises GsError (code -4: a stream this path does not take -- the host decoders do; -1: a damaged stream)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    out = np.zeros(max(int(expect_bytes), 1), dtype=np.uint8)
    n = C.c_int64(0)
    info = (C.c_int64 * 4)()
    rc = lib().gs_gunzip_device(device, buf.ctypes.data_as(C.c_void_p), len(buf), out.ctypes.data_as(C.c_void_p), int(expect_bytes), C.byref(n), info)
    if rc != 0:
        raise GsError(rc, (lib().gs_inflate_last_error() or b"").decode(errors="replace"))
    return out[:n.value], list(info)


def _fetch_device(device, p, n):
    out = np.zeros(max(n, 1), dtype=np.uint8)
    if n:
        rc = lib().gs_device_fetch(device, p, out.ctypes.data_as(C.c_void_p), n)
        if rc != 0:
            raise GsError(rc, (lib().gs_inflate_last_error() or b"").decode(errors="replace"))
    return out[:n]


def _deflate(fn, data, *head):
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    cap = int(lib().gs_deflate_bound(len(buf))) + 64
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_int64(0)
    rc = fn(*head, buf.ctypes.data_as(C.c_void_p) if len(buf) else None, len(buf), out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    if rc != 0:
        raise GsError(rc, (lib().gs_deflate_last_error() or b"").decode(errors="replace"))
    return out[:n.value]


def deflate_device(data, device=0):
    """gs_deflate_host: bytes -> BGZF members written on the device (numpy uint8; no end-of-file block)"""
    return _deflate(lib().gs_deflate_host, data, device)


def deflate_reference(data):
    """gs_deflate_host_reference: the same format from the CPU loop over the same table builder (no device)"""
    return _deflate(lib().gs_deflate_host_reference, data)


class DeviceDeflater:
    """gs_deflater_*: device text -> BGZF members in a (page-locked) host buffer"""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        self.device = device
        rc = lib().gs_deflater_create(C.byref(self.h), device)
        if rc != 0:
            raise GsError(rc, (lib().gs_deflate_last_error() or b"").decode(errors="replace"))

    def pack(self, d_text, n, out):
        """d_text: device pointer (int) or tensor with data_ptr(); out: numpy uint8 of at least gs_deflate_bound(n) bytes -> bytes written"""
        p = C.c_void_p(d_text.data_ptr() if hasattr(d_text, "data_ptr") else int(d_text))
        _ready(d_text)
        n_out = C.c_int64(0)
        rc = lib().gs_deflater_pack(self.h, p, int(n), out.ctypes.data_as(C.c_void_p), int(out.shape[0]), C.byref(n_out))
        if rc != 0:
            raise GsError(rc, (lib().gs_deflate_last_error() or b"").decode(errors="replace"))
        return n_out.value

    def append(self, d_text, n):
        """gs_deflater_append: the text waits on the device for flush()"""
        p = C.c_void_p(d_text.data_ptr() if hasattr(d_text, "data_ptr") else int(d_text))
        _ready(d_text)
        rc = lib().gs_deflater_append(self.h, p, int(n))
        if rc != 0:
            raise GsError(rc, (lib().gs_deflate_last_error() or b"").decode(errors="replace"))

    def pending(self):
        return int(lib().gs_deflater_pending(self.h))

    def flush(self):
        """the waiting text as BGZF members (numpy uint8)"""
        out = np.empty(deflate_bound(self.pending()), dtype=np.uint8)
        n_out = C.c_int64(0)
        rc = lib().gs_deflater_flush(self.h, out.ctypes.data_as(C.c_void_p), int(out.shape[0]), C.byref(n_out))
        if rc != 0:
            raise GsError(rc, (lib().gs_deflate_last_error() or b"").decode(errors="replace"))
        return out[:n_out.value]

    def close(self):
        if getattr(self, "h", None):
            lib().gs_deflater_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def deflate_bound(n):
    return int(lib().gs_deflate_bound(int(n)))


BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


CAL_VALU_PURE, CAL_VALU_MIX, CAL_SALU, CAL_VALU_SALU = 0, 1, 2, 3
CAL_VMEM_BYTES, CAL_VMEM_WORDS, CAL_VMEM_SHARED_LINES, CAL_VMEM_SCATTERED, CAL_RANDOM_LINES = 4, 5, 6, 7, 8


def calibrate(what, arg=0, device=0):
    """gs_calibrate: a measured ceiling of the device (include/gsgpu.h) -> dict(rate, ms, count, n_cu)"""
    out = (C.c_double * 4)()
    _check(lib().gs_calibrate(device, what, arg, out))
    return {"rate": out[0], "ms": out[1], "count": out[2], "n_cu": int(out[3])}


def _ptr(a):
    """(pointer, mem kind) of a numpy array (host) or a tensor-like with data_ptr() (device)"""
    if a is None:
        return None, None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(C.c_void_p), MEM_HOST
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr()), (MEM_DEVICE if getattr(a, "is_cuda", True) else MEM_HOST)
    raise TypeError(f"unsupported buffer {type(a)}")


def _ready(*bufs):
    """The library works on its own HIP stream and takes device buffers as complete (include/gsgpu.h): wait for the
    producer's stream (torch's current one) before handing tensors over."""
    torch = sys.modules.get("torch")
    if torch is None:
        return
    for b in bufs:
        if isinstance(b, DeviceView):  # (memory of one of the library's own handles: complete when the handle hands it out)
            continue
        if b is not None and getattr(b, "is_cuda", False):
            torch.cuda.current_stream(b.device).synchronize()
            return


class DeviceKMerStore:
    """k-mer -> value-index store plus taxonomy, resident in HBM (gs_db)."""

    def __init__(self, k, kmers_sorted, value_idx, n_values, parent_vi=None, device=0, n_parts=1, part=0,
                 partition=None):
        """partition: build a partition store for the split pipeline encode -> probe_keys -> reduce (gs_db_create_part:
        every key in the table); default: n_parts > 1.  Otherwise the store serves the fused kernels (gs_db_create)."""
        kmers = np.ascontiguousarray(kmers_sorted, dtype=np.int64)
        vidx = np.ascontiguousarray(value_idx, dtype=np.int32)
        if len(kmers) != len(vidx):
            raise ValueError("kmers / value_idx length mismatch")
        pv = None if parent_vi is None else np.ascontiguousarray(parent_vi, dtype=np.int32)
        if pv is not None and len(pv) != n_values:
            raise ValueError("parent_vi must have n_values entries")
        self.h = C.c_void_p()
        self.k, self.n_values, self.device = k, n_values, device
        if partition is None:
            partition = n_parts > 1
        if partition:
            _check(lib().gs_db_create_part(C.byref(self.h), device, k, len(kmers), kmers.ctypes.data_as(C.c_void_p),
                                           vidx.ctypes.data_as(C.c_void_p), n_values,
                                           None if pv is None else pv.ctypes.data_as(C.c_void_p), n_parts, part))
        else:
            _check(lib().gs_db_create(C.byref(self.h), device, k, len(kmers), kmers.ctypes.data_as(C.c_void_p),
                                      vidx.ctypes.data_as(C.c_void_p), n_values,
                                      None if pv is None else pv.ctypes.data_as(C.c_void_p)))

    @staticmethod
    def _arrays(kmers, value_idx, n_values, parent_vi):
        kmers = np.ascontiguousarray(kmers, dtype=np.int64)
        vidx = np.ascontiguousarray(value_idx, dtype=np.int32)
        if len(kmers) != len(vidx):
            raise ValueError("kmers / value_idx length mismatch")
        pv = None if parent_vi is None else np.ascontiguousarray(parent_vi, dtype=np.int32)
        if pv is not None and len(pv) != n_values:
            raise ValueError("parent_vi must have n_values entries")
        return kmers, vidx, pv

    @classmethod
    def _wrap(cls, h, k, n_values, device):
        self = cls.__new__(cls)
        self.h, self.k, self.n_values, self.device = h, k, n_values, device
        return self

    @classmethod
    def striped(cls, k, kmers, value_idx, n_values, parent_vi=None, devices=(0, 0)):
        """gs_db_create_striped: ONE record table split over `devices` (stripe p in the HBM of devices[p]; a device may
        repeat), gates / overflow table / tree on each.  Returns one handle per stripe; every handle serves the fused
        kernels on its device and reads foreign stripes over peer access."""
        kmers, vidx, pv = cls._arrays(kmers, value_idx, n_values, parent_vi)
        n = len(devices)
        out = (C.c_void_p * n)()
        dev = (C.c_int * n)(*devices)
        _check(lib().gs_db_create_striped(out, dev, n, k, len(kmers), kmers.ctypes.data_as(C.c_void_p),
                                          vidx.ctypes.data_as(C.c_void_p), n_values,
                                          None if pv is None else pv.ctypes.data_as(C.c_void_p)))
        return [cls._wrap(C.c_void_p(out[p]), k, n_values, devices[p]) for p in range(n)]

    @classmethod
    def stripe(cls, k, kmers, value_idx, n_values, parent_vi=None, device=0, n_stripes=2, stripe=0):
        """gs_db_create_stripe: this process's stripe of a striped store (one process per GPU); the other stripes are
        attached from their owners' handles: export_stripe() -> all-gather -> attach_stripe()
        (genestrip_amd.distributed.striped_store does all of it)."""
        kmers, vidx, pv = cls._arrays(kmers, value_idx, n_values, parent_vi)
        h = C.c_void_p()
        _check(lib().gs_db_create_stripe(C.byref(h), device, n_stripes, stripe, k, len(kmers), kmers.ctypes.data_as(C.c_void_p),
                                         vidx.ctypes.data_as(C.c_void_p), n_values,
                                         None if pv is None else pv.ctypes.data_as(C.c_void_p)))
        return cls._wrap(h, k, n_values, device)

    @classmethod
    def load_striped(cls, path, devices=(0, 0)):
        """gs_db_load_striped: a store file (save() of a plain store) into the HBM of `devices`, one stripe each"""
        n = len(devices)
        out = (C.c_void_p * n)()
        _check(lib().gs_db_load_striped(out, (C.c_int * n)(*devices), n, str(path).encode()))
        res = []
        for p in range(n):
            s = cls._wrap(C.c_void_p(out[p]), 0, 0, devices[p])
            i = s.info
            s.k, s.n_values = i.k, i.n_values
            res.append(s)
        return res

    @classmethod
    def load_stripe(cls, path, device=0, n_stripes=2, stripe=0):
        """gs_db_load_stripe: this process's stripe of a store file (then export_stripe / attach_stripe as for stripe())"""
        h = C.c_void_p()
        _check(lib().gs_db_load_stripe(C.byref(h), device, n_stripes, stripe, str(path).encode()))
        s = cls._wrap(h, 0, 0, device)
        i = s.info
        s.k, s.n_values = i.k, i.n_values
        return s

    def export_stripe(self):
        buf = C.create_string_buffer(64)
        _check(lib().gs_db_stripe_export(self.h, buf))
        return buf.raw

    def attach_stripe(self, stripe, handle):
        _check(lib().gs_db_stripe_attach(self.h, stripe, C.c_char_p(bytes(handle))))

    @classmethod
    def load(cls, path, device=0):
        """open a native store file written by save() (gs_db_load)"""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        _check(lib().gs_db_load(C.byref(self.h), device, str(path).encode()))
        self.device = device
        i = self.info
        self.k, self.n_values = i.k, i.n_values
        return self

    def save(self, path):
        _check(lib().gs_db_save(self.h, str(path).encode()))

    @property
    def info(self):
        i = DbInfo()
        _check(lib().gs_db_get_info(self.h, C.byref(i)))
        return i

    def export(self, select=None, with_desc=True):
        """KMerStore.visit (gs_dbexport_create + _fetch): the stored (k-mer, value index) pairs of this handle in ascending k-mer
        order -> (kmers int64, value_idx int32).  select = a value index: only that value (with_desc=False) or its subtree
        (with_desc=True); None: all.  What comes back is the n_stored pairs: reachable ones whose value has a tree node."""
        x = C.c_void_p()
        n = C.c_int64(0)
        _check(lib().gs_dbexport_create(C.byref(x), self.h, -1 if select is None else int(select), int(bool(with_desc)), C.byref(n)))
        try:
            kmers = np.empty(n.value, dtype=np.int64)
            vals = np.empty(n.value, dtype=np.int32)
            _check(lib().gs_dbexport_fetch(x, kmers.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), MEM_HOST))
        finally:
            lib().gs_dbexport_destroy(x)
        return kmers, vals

    def value_counts(self):
        """Database.getStats per value index (gs_db_value_counts): stored k-mers of each value, int64[n_values]"""
        out = np.zeros(self.info.n_values, dtype=np.int64)
        _check(lib().gs_db_value_counts(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().gs_db_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kmer_ranges(k, n):
    """n ranges [lo, hi) of the canonical k-mer with about equal shares of the k-mers (a canonical k-mer is the larger of
    two strands: P(x <= t) ~ (t / 4^k)^2): for gs_dbbuild_set_range.  This assumes k-mers spread evenly over the key space and
    needs no pass over the data: good for a first cut or for random sequence.  Genomes are not like that (poly-A, repeats, GC
    skew), and n itself is a guess: when the collection can be walked once first, prefer plan_ranges() over the histogram of a
    DeviceDbSizer, which bounds every range by what it really holds."""
    import math
    top = 1 << (2 * k)
    cuts = [math.isqrt(top * top * i // n) for i in range(n)] + [top]
    return [(cuts[i], cuts[i + 1]) for i in range(n) if cuts[i] < cuts[i + 1]]


def plan_ranges(hist, hist_bits, k, max_pairs):
    """gs_dbsize_plan: the fewest ranges [lo, hi) of the canonical k-mer, cut at the bins of a DeviceDbSizer histogram, that
    hold at most max_pairs k-mers each (max_pairs = the device memory granted / 40 for DeviceDbBuilder, / 24 for
    DeviceDbQuality).  Histograms are additive: add those of fill and update regions first.  Needs no device.  A single bin above
    max_pairs raises GsError (more hist_bits split it)."""
    if not 1 <= k <= 31 or not 1 <= hist_bits <= 12:
        raise ValueError("k must be in [1, 31] and hist_bits in [1, 12]")
    bins = 1 << min(hist_bits, 2 * k)
    h = np.ascontiguousarray(hist, dtype=np.int64)
    if h.shape != (bins,):
        raise ValueError(f"hist must have {bins} entries")
    bounds = np.zeros(bins + 1, dtype=np.uint64)
    n = C.c_int(0)
    _check(lib().gs_dbsize_plan(h.ctypes.data_as(C.c_void_p), hist_bits, k, int(max_pairs), bounds.ctypes.data_as(C.c_void_p), bins,
                                C.byref(n)))
    return [(int(bounds[i]), int(bounds[i + 1])) for i in range(n.value)]


def _region_args(seq, offsets, per_region, name):
    """a batch of regions for gs_dbbuild_add / gs_dbquality_add / gs_dbupdate_add / gs_dbsize_add -> (seq pointer, offsets pointer, tags int32[n], n, mem)"""
    ps, mem = _ptr(seq)
    po, mem2 = _ptr(offsets)
    assert mem == mem2, "seq and offsets must live in the same memory space"
    tags = np.ascontiguousarray(per_region, dtype=np.int32)
    n = (offsets.shape[0] if hasattr(offsets, "shape") else len(offsets)) - 1
    if len(tags) != n:
        raise ValueError(f"{name} must have one entry per region")
    _ready(seq, offsets)
    return ps, po, tags, n, mem


class DeviceDbBuilder:
    """gs_dbbuild: distinct canonical k-mers of genome regions with the LCA of the nodes that hold them (FillDBGoal + DBGoal)"""

    def __init__(self, k, n_values, parent_vi, device=0, lower_case_bases=True, max_dust=-1, step_size=1):
        pv = np.ascontiguousarray(parent_vi, dtype=np.int32)
        if len(pv) != n_values:
            raise ValueError("parent_vi must have n_values entries")
        self.h = C.c_void_p()
        self.k, self.n_values = k, n_values
        _check(lib().gs_dbbuild_begin(C.byref(self.h), device, k, n_values, pv.ctypes.data_as(C.c_void_p), int(lower_case_bases),
                                      max_dust, step_size))

    def set_range(self, lo, hi):
        """keep only the canonical k-mers in [lo, hi) (before the first add): one builder per range of kmer_ranges()"""
        _check(lib().gs_dbbuild_set_range(self.h, lo, hi))

    def add(self, seq, offsets, node_vi, update=False):
        """regions: seq (uint8) + offsets (uint64, n + 1, from 0), both numpy or both device tensors; node_vi: numpy int32[n]"""
        ps, po, tags, n, mem = _region_args(seq, offsets, node_vi, "node_vi")
        _check(lib().gs_dbbuild_add(self.h, ps, po, tags.ctypes.data_as(C.c_void_p), n, mem, int(update)))

    def finish(self):
        """-> (kmers int64 ascending, value_idx int32): what DeviceKMerStore takes"""
        n = C.c_int64(0)
        _check(lib().gs_dbbuild_finish(self.h, C.byref(n)))
        kmers = np.zeros(n.value, dtype=np.int64)
        vals = np.zeros(n.value, dtype=np.int32)
        _check(lib().gs_dbbuild_fetch(self.h, kmers.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p)))
        return kmers, vals

    def finish_count(self):
        """sort + fold only: the number of stored k-mers (the arrays stay on the device: fetch() or to_store())"""
        n = C.c_int64(0)
        _check(lib().gs_dbbuild_finish(self.h, C.byref(n)))
        return n.value

    def to_store(self, device=0):
        """gs_dbbuild_to_db: the store over the built arrays, laid out on the device, nothing through the host"""
        self.finish_count()
        h = C.c_void_p()
        _check(lib().gs_dbbuild_to_db(self.h, C.byref(h)))
        return DeviceKMerStore._wrap(h, self.k, self.n_values, device)

    def close(self):
        if getattr(self, "h", None):
            lib().gs_dbbuild_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DbQualityStats(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("n_distinct", C.c_int64), ("n_found", C.c_int64), ("n_store", C.c_int64),
                ("ms_pairs", C.c_double), ("ms_sort", C.c_double), ("ms_decode", C.c_double), ("ms_join", C.c_double)]


class DeviceDbQuality:
    """gs_dbquality: per leaf value index tp / tp+fp / tp+fn of a store against its source genomes (the reference's dbqualcounts
    goal, DBQualityCountsGoal.handleStore): k-mers are formed as in DeviceDbBuilder, de-duplicated exactly per (k-mer, leaf) and
    looked up in the store on the device"""

    def __init__(self, store, lower_case_bases=True, max_dust=-1, step_size=1):
        self.store = store  # (the handle reads the store until close())
        self.n_values = store.n_values
        self.h = C.c_void_p()
        _check(lib().gs_dbquality_begin(C.byref(self.h), store.h, int(lower_case_bases), max_dust, step_size))

    def set_range(self, lo, hi):
        """keep only the canonical k-mers in [lo, hi): before the first add of a pass; after finish() it starts the next pass
        on this handle (one pass per range of kmer_ranges(); add the tp / tp+fn columns of the passes)"""
        _check(lib().gs_dbquality_set_range(self.h, lo, hi))

    def add(self, seq, offsets, leaf_vi):
        """regions as for DeviceDbBuilder.add; leaf_vi: numpy int32[n], negative = the region counts nothing"""
        ps, po, tags, n, mem = _region_args(seq, offsets, leaf_vi, "leaf_vi")
        _check(lib().gs_dbquality_add(self.h, ps, po, tags.ctypes.data_as(C.c_void_p), n, mem))

    def finish(self):
        """-> (counts int64[n_values, 3]: tp, tp+fp, tp+fn; present uint8[n_values]): rows with present == 0 are absent"""
        counts = np.zeros((self.n_values, 3), dtype=np.int64)
        present = np.zeros(self.n_values, dtype=np.uint8)
        _check(lib().gs_dbquality_finish(self.h, counts.ctypes.data_as(C.c_void_p), present.ctypes.data_as(C.c_void_p)))
        return counts, present

    def stats(self):
        """sizes and phase times (ms) of the latest pass"""
        st = DbQualityStats()
        _check(lib().gs_dbquality_get_stats(self.h, C.byref(st)))
        return st

    def close(self):
        if getattr(self, "h", None):
            lib().gs_dbquality_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DbUpdateStats(C.Structure):
    _fields_ = [("n_store", C.c_int64), ("n_pairs", C.c_int64), ("n_found", C.c_int64), ("n_moved", C.c_int64),
                ("store_bytes", C.c_int64), ("batch_bytes_peak", C.c_int64),
                ("ms_begin", C.c_double), ("ms_kmers", C.c_double), ("ms_lookup", C.c_double), ("ms_finish", C.c_double)]


class DeviceDbUpdater:
    """gs_dbupdate: a finished store updated in batches (the reference's updatedb stage, DBGoal.MyFastaReader): every stored
    k-mer that occurs in an added region gets value := LCA(value, node of the region).  The store stays on the device, the
    regions stream past it in slices: memory does not grow with the number of add() calls, and their order does not matter."""

    def __init__(self):
        raise TypeError("use DeviceDbUpdater.from_arrays / from_store / from_builder")

    @classmethod
    def _new(cls, k, n_values, device):
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self.k, self.n_values, self.device = k, n_values, device
        return self

    @classmethod
    def from_arrays(cls, k, kmers, value_idx, n_values, parent_vi, device=0, lower_case_bases=True, max_dust=-1, step_size=1):
        """the arrays DeviceDbBuilder.finish() returns / DeviceKMerStore takes: both numpy or both device tensors"""
        pv = np.ascontiguousarray(parent_vi, dtype=np.int32)
        if len(pv) != n_values:
            raise ValueError("parent_vi must have n_values entries")
        if isinstance(kmers, np.ndarray) or not hasattr(kmers, "data_ptr"):
            kmers = np.ascontiguousarray(kmers, dtype=np.int64)
            value_idx = np.ascontiguousarray(value_idx, dtype=np.int32)
        n = kmers.shape[0]
        if value_idx.shape[0] != n:
            raise ValueError("kmers / value_idx length mismatch")
        pk, mem = _ptr(kmers)
        pvl, mem2 = _ptr(value_idx)
        assert mem == mem2, "kmers and value_idx must live in the same memory space"
        _ready(kmers, value_idx)
        self = cls._new(k, n_values, device)
        _check(lib().gs_dbupdate_begin(C.byref(self.h), device, k, n_values, pv.ctypes.data_as(C.c_void_p), int(lower_case_bases),
                                       max_dust, step_size, pk, pvl, n, mem))
        return self

    @classmethod
    def from_store(cls, store, lower_case_bases=True, max_dust=-1, step_size=1):
        """the k-mers of a live DeviceKMerStore (decoded on the device; the store is only read and may be closed afterwards)"""
        self = cls._new(store.k, store.n_values, store.device)
        _check(lib().gs_dbupdate_begin_db(C.byref(self.h), store.h, int(lower_case_bases), max_dust, step_size))
        return self

    @classmethod
    def from_builder(cls, builder, device=0):
        """the result of a DeviceDbBuilder (finished here if it is not yet); its parameters are inherited and it keeps its own
        arrays"""
        builder.finish_count()
        self = cls._new(builder.k, builder.n_values, device)
        _check(lib().gs_dbupdate_begin_build(C.byref(self.h), builder.h))
        return self

    def set_slice(self, max_bases):
        """a batch is worked off in slices of at most max_bases bases (at least k - 1 + step_size); results do not change"""
        _check(lib().gs_dbupdate_set_slice(self.h, int(max_bases)))

    def add(self, seq, offsets, node_vi):
        """regions as for DeviceDbBuilder.add(..., update=True)"""
        ps, po, tags, n, mem = _region_args(seq, offsets, node_vi, "node_vi")
        _check(lib().gs_dbupdate_add(self.h, ps, po, tags.ctypes.data_as(C.c_void_p), n, mem))

    def finish(self):
        """-> the number of stored k-mers whose value differs from the value at the start; no add() afterwards"""
        n = C.c_int64(0)
        _check(lib().gs_dbupdate_finish(self.h, C.byref(n)))
        return n.value

    def fetch(self):
        """-> (kmers int64 ascending, value_idx int32) after finish()"""
        n = self.stats().n_store
        kmers = np.zeros(n, dtype=np.int64)
        vals = np.zeros(n, dtype=np.int32)
        _check(lib().gs_dbupdate_fetch(self.h, kmers.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p)))
        return kmers, vals

    def to_store(self):
        """gs_dbupdate_to_db: the store over the updated arrays, laid out on the device, nothing through the host"""
        h = C.c_void_p()
        _check(lib().gs_dbupdate_to_db(self.h, C.byref(h)))
        return DeviceKMerStore._wrap(h, self.k, self.n_values, self.device)

    def stats(self):
        """counts so far, device bytes and phase times (ms)"""
        st = DbUpdateStats()
        _check(lib().gs_dbupdate_get_stats(self.h, C.byref(st)))
        return st

    def close(self):
        if getattr(self, "h", None):
            lib().gs_dbupdate_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DbSizeTotals(C.Structure):
    _fields_ = [("total", C.c_int64), ("dust", C.c_int64), ("included", C.c_int64)]


class DbSizeStats(C.Structure):
    _fields_ = [("n_bases", C.c_int64), ("n_regions", C.c_int64), ("n_keys", C.c_int64), ("n_distinct", C.c_int64),
                ("bytes_fixed", C.c_int64), ("batch_bytes_peak", C.c_int64), ("bytes_peak", C.c_int64),
                ("ms_add", C.c_double), ("ms_count", C.c_double), ("ms_sort", C.c_double), ("ms_heads", C.c_double),
                ("n_values", C.c_int32), ("hist_bins", C.c_int32), ("radix_bits", C.c_int32), ("keep_keys", C.c_int32)]


class DeviceDbSizer:
    """gs_dbsize: a genome collection sized before it is built (the reference's fillsize and tempindex walks, FillSizeGoal +
    FillBloomFilterGoal): k-mers with duplicates, those the DUST gate drops, those that remain, per tag and as a histogram of
    the canonical k-mer's top bits (plan_ranges); with keep_keys the distinct k-mers, exactly, in total and per radix bucket.
    K-mers are formed as in DeviceDbBuilder; the handle takes no tree, tags are plain indices in [0, n_values)."""

    def __init__(self, k, n_values=1, device=0, lower_case_bases=True, max_dust=-1, step_size=1, hist_bits=12, radix_bits=0,
                 keep_keys=False):
        if not 1 <= hist_bits <= 12:
            raise ValueError("hist_bits must be in [1, 12]")
        if radix_bits != 0 and not 16 <= radix_bits <= 24:
            raise ValueError("radix_bits must be 0 or in [16, 24]")
        self.h = C.c_void_p()
        self.k, self.n_values, self.hist_bits = k, n_values, hist_bits
        self.radix_bits = radix_bits if keep_keys else 0
        _check(lib().gs_dbsize_begin(C.byref(self.h), device, k, n_values, int(lower_case_bases), max_dust, step_size, hist_bits,
                                     radix_bits, int(keep_keys)))

    def set_range(self, lo, hi):
        """retain only the canonical k-mers in [lo, hi) (the counts always cover every k-mer): before the first add, or after
        counts() / distinct() to start the next pass on this handle with every counter at zero"""
        _check(lib().gs_dbsize_set_range(self.h, lo, hi))

    def add(self, seq, offsets, tag_vi):
        """regions as for DeviceDbBuilder.add; tag_vi: numpy int32[n] in [0, n_values)"""
        ps, po, tags, n, mem = _region_args(seq, offsets, tag_vi, "tag_vi")
        _check(lib().gs_dbsize_add(self.h, ps, po, tags.ctypes.data_as(C.c_void_p), n, mem))

    def counts(self):
        """-> (DbSizeTotals: total, dust, included; per_value int64[n_values]; hist int64[1 << min(hist_bits, 2k)])"""
        t = DbSizeTotals()
        per_value = np.zeros(self.n_values, dtype=np.int64)
        hist = np.zeros(1 << min(self.hist_bits, 2 * self.k), dtype=np.int64)
        _check(lib().gs_dbsize_counts(self.h, C.byref(t), per_value.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p)))
        return t, per_value, hist

    def distinct(self):
        """-> (number of distinct retained k-mers, bucket_sizes int64[1 << radix_bits] or None); releases the keys"""
        n = C.c_int64(0)
        buckets = np.zeros(1 << self.radix_bits, dtype=np.int64) if self.radix_bits else None
        _check(lib().gs_dbsize_distinct(self.h, C.byref(n), None if buckets is None else buckets.ctypes.data_as(C.c_void_p)))
        return n.value, buckets

    def stats(self):
        """sizes, device bytes and phase times (ms) of the pass"""
        st = DbSizeStats()
        _check(lib().gs_dbsize_get_stats(self.h, C.byref(st)))
        return st

    def close(self):
        if getattr(self, "h", None):
            lib().gs_dbsize_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceView:
    """a device array that belongs to a handle of the library: what _ptr / _region_args take in place of a tensor (is_cuda says
    where it lives; no torch stream is involved, the handle has synchronised its own)"""
    is_cuda = True

    def __init__(self, ptr, n, dtype, device):
        self.ptr, self.shape, self.dtype, self.device = ptr, (n,), np.dtype(dtype), device

    def data_ptr(self):
        return self.ptr

    def numpy(self):
        """a host copy"""
        raw = _fetch_device(self.device, C.c_void_p(self.ptr), self.shape[0] * self.dtype.itemsize)
        return raw.view(self.dtype).copy()


class DeviceGenomes:
    """gs_genomes: genome FASTA text to the regions of a build.  scan() finds the records of a chunk, headers() hands their header
    lines to the caller, gather() takes one keep flag per record and leaves the bases of the kept records on the device, regions()
    is what DeviceDbBuilder / DeviceDbSizer / DeviceDbUpdater / DeviceDbQuality .add take.  A chunk with a NUL byte or a run of
    more than 64 '\r' raises GsError(-4): it belongs to the host parser (host.genome_files does that)."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        self.device = device
        self.n_records = self.n_regions = self.n_bases = self.header_bytes = 0
        _check(lib().gs_genomes_create(C.byref(self.h), device))

    def scan(self, text, last=True):
        """text: bytes, numpy uint8 or a device tensor of uint8 -> (n_records, consumed_bytes, header_bytes, max_line_bytes)"""
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(text, dtype=np.uint8)
        n = int(text.shape[0])
        p, mem = _ptr(text) if n else (None, MEM_HOST)
        _ready(text)
        out = [C.c_int64(0) for _ in range(4)]
        self.n_records = self.n_regions = self.n_bases = self.header_bytes = 0
        _check(lib().gs_genomes_scan(self.h, p, n, mem, int(bool(last)), *[C.byref(o) for o in out]))
        self.n_records, self.header_bytes = out[0].value, out[2].value
        return tuple(o.value for o in out)

    def headers(self):
        """-> (headers uint8, header_off uint64[n_records + 1])"""
        hdr = np.zeros(max(self.header_bytes, 1), dtype=np.uint8)
        off = np.zeros(self.n_records + 1, dtype=np.uint64)
        _check(lib().gs_genomes_headers(self.h, hdr.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p)))
        return hdr[:self.header_bytes], off

    def gather(self, keep=None):
        """keep: one flag per record (None: all) -> (n_regions, n_bases)"""
        pk = None
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
            if len(keep) != self.n_records:
                raise ValueError("keep must have one entry per record")
            pk = keep.ctypes.data_as(C.c_void_p)
        nr, nb = C.c_int64(0), C.c_int64(0)
        _check(lib().gs_genomes_gather(self.h, pk, C.byref(nr), C.byref(nb)))
        self.n_regions, self.n_bases = nr.value, nb.value
        return nr.value, nb.value

    def regions(self):
        """-> (seq, offsets) on the device, valid until the next scan / gather / close"""
        ps, po = C.c_void_p(), C.c_void_p()
        _check(lib().gs_genomes_regions(self.h, C.byref(ps), C.byref(po)))
        return DeviceView(ps.value, self.n_bases, np.uint8, self.device), DeviceView(po.value, self.n_regions + 1, np.uint64, self.device)

    def kernel_time(self):
        """-> (ms of the scan kernels, ms of the select and gather kernels) so far"""
        a, b = C.c_double(0), C.c_double(0)
        _check(lib().gs_genomes_kernel_time(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            lib().gs_genomes_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge_runs(matchers):
    """gs_match_merge: the runs of one process (one per GPU, or several on one GPU) into a global state held by each"""
    arr = (C.c_void_p * len(matchers))(*[m.h for m in matchers])
    _check(lib().gs_match_merge(arr, len(matchers)))


class MatchConfig:
    """the GSConfigKey values that parameterise matchRead (C/GSConfigKey.java:302-350)"""

    def __init__(self, classify=True, count_unique=True, max_paths=10, threshold=1, max_read_tax_err=-1.0,
                 max_read_class_err=-1.0, profile=False, max_kmer_res_counts=0):
        self.classify, self.count_unique, self.max_paths, self.threshold = classify, count_unique, max_paths, threshold
        self.max_read_tax_err, self.max_read_class_err, self.profile = max_read_tax_err, max_read_class_err, profile
        self.max_kmer_res_counts = max_kmer_res_counts

    def _c(self):
        return _MatchCfg(int(self.classify), int(self.count_unique), self.max_paths, self.threshold,
                         self.max_read_tax_err, self.max_read_class_err, int(self.profile), int(self.max_kmer_res_counts))


class FastqKMerMatcher:
    """one runMatcher() scope: begin -> submit batches -> finish."""

    def __init__(self, store, config=None):
        self.store = store
        self.config = config or MatchConfig()
        cfg = self.config._c()
        self.h = C.c_void_p()
        _check(lib().gs_match_begin(C.byref(self.h), store.h, C.byref(cfg)))

    def submit(self, seq, offsets, first_read_no=0, class_vi=None, flags=None, n_reads=None):
        ps, mem = _ptr(seq)
        po, mem2 = _ptr(offsets)
        assert mem == mem2, "seq and offsets must live in the same memory space"
        if n_reads is None:
            n_reads = (offsets.shape[0] if hasattr(offsets, "shape") else len(offsets)) - 1
        pc, _ = _ptr(class_vi)
        pf, _ = _ptr(flags)
        _ready(seq, offsets, class_vi, flags)
        _check(lib().gs_match_submit(self.h, ps, po, n_reads, first_read_no, mem, pc, pf))

    def submit_fixed(self, seq, read_len, n_reads, first_read_no=0, class_vi=None, flags=None):
        """gs_match_submit_fixed: n_reads reads of read_len bytes each, back to back in `seq` (numpy = host, tensor = device)"""
        ps, mem = _ptr(seq)
        pc, _ = _ptr(class_vi)
        pf, _ = _ptr(flags)
        _ready(seq, class_vi, flags)
        _check(lib().gs_match_submit_fixed(self.h, ps, int(read_len), int(n_reads), int(first_read_no), mem, pc, pf))

    def submit_async(self, seq, offsets, first_read_no=0, class_vi=None, flags=None, n_reads=None):
        """host batch (numpy arrays, best page-locked), queued: returns a ticket for wait(); the arrays must stay as they
        are until then.  Two batches can be under way (gs_match_submit_async)."""
        ps, mem = _ptr(seq)
        po, mem2 = _ptr(offsets)
        assert mem == mem2 == MEM_HOST, "submit_async takes host arrays"
        if n_reads is None:
            n_reads = (offsets.shape[0] if hasattr(offsets, "shape") else len(offsets)) - 1
        pc, _ = _ptr(class_vi)
        pf, _ = _ptr(flags)
        ticket = C.c_int64(-1)
        _check(lib().gs_match_submit_async(self.h, ps, po, n_reads, first_read_no, pc, pf, C.byref(ticket)))
        return ticket.value

    def wait(self, ticket):
        _check(lib().gs_match_wait(self.h, ticket))

    def match_reads(self, seq, offsets, first_read_no=0):
        """host batch -> (class_vi, flags) numpy arrays (the per-read outcome of matchRead)"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        cv = np.full(n, -1, dtype=np.int32)
        fl = np.zeros(n, dtype=np.uint8)
        if len(seq) == 0:
            seq = np.zeros(1, dtype=np.uint8)
        self.submit(seq, offsets, first_read_no, cv, fl)
        return cv, fl

    def submit_text(self, text, n_lines=None, first_read_no=0, class_vi=None, flags=None):
        """raw FASTQ text of whole 4-line records (numpy uint8 / bytes on the host, or a device tensor): the records
        are found on the device (gs_match_submit_text).  Returns the ticket."""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        if n_lines is None:
            n_lines = int((text == 10).sum())
        n_bytes = int(text.shape[0])
        pt, mem = _ptr(text) if n_bytes else (None, MEM_HOST)
        pc, _ = _ptr(class_vi)
        pf, _ = _ptr(flags)
        _ready(text, class_vi, flags)
        ticket = C.c_int64(-1)
        self._text_keep = text  # the copy is asynchronous
        self._text_reads = int(n_lines) // 4
        _check(lib().gs_match_submit_text(self.h, pt, n_bytes, int(n_lines), mem, first_read_no, pc, pf, C.byref(ticket)))
        return ticket.value

    def submit_fasta(self, text, n_lines=None, n_records=None, first_read_no=0, class_vi=None, flags=None):
        """raw FASTA text of whole records (gs_match_submit_fasta); returns the ticket"""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n_bytes = int(text.shape[0])
        if n_lines is None or n_records is None:
            host = text if isinstance(text, np.ndarray) else text.cpu().numpy()
            nl = np.flatnonzero(host == 10)
            starts = np.concatenate([[0], nl[:-1] + 1]) if len(nl) else np.zeros(0, dtype=np.int64)
            n_lines = len(nl) if n_lines is None else n_lines
            n_records = int((host[starts] == ord(">")).sum()) if n_records is None else n_records
        pt, mem = _ptr(text) if n_bytes else (None, MEM_HOST)
        pc, _ = _ptr(class_vi)
        pf, _ = _ptr(flags)
        _ready(text, class_vi, flags)
        ticket = C.c_int64(-1)
        self._text_keep = text
        _check(lib().gs_match_submit_fasta(self.h, pt, n_bytes, int(n_lines), int(n_records), mem, first_read_no, pc, pf,
                                           C.byref(ticket)))
        return ticket.value

    def submit_fastq_ml(self, text, n_lines=None, first_read_no=0, class_vi=None, flags=None):
        """general FASTQ text (sequence / quality over any number of lines) starting at a descriptor line: -> (records matched,
        bytes they cover); the rest belongs in front of the next chunk (gs_match_submit_fastq_ml).  class_vi / flags: room for
        n_lines // 4 + 1 records"""
        pt, mem = _ptr(text)
        n_bytes = int(text.shape[0] if hasattr(text, "shape") else len(text))
        if n_lines is None:
            n_lines = int(np.count_nonzero(np.asarray(text) == 10)) if mem == MEM_HOST else int((text == 10).sum().item())
        n_rec, used, ticket = C.c_int64(0), C.c_int64(0), C.c_int64(-1)
        pc, _ = _ptr(class_vi)
        pf, _ = _ptr(flags)
        _ready(text, class_vi, flags)
        self._text_keep = text
        _check(lib().gs_match_submit_fastq_ml(self.h, pt, n_bytes, n_lines, mem, first_read_no, pc, pf, C.byref(n_rec), C.byref(used),
                                              None, C.byref(ticket)))
        self._text_reads = max(n_rec.value, 0)
        return max(n_rec.value, 0), used.value

    def compact_text(self, with_probs=False, slot=0):
        """gs_match_compact_text: the reads of the last four-line chunk that matchRead returned true for, as afterMatch writes them,
        gathered on the device -> (bytes as numpy uint8, records)"""
        p, nb, nr, d = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int(0)
        _check(lib().gs_match_compact_text(self.h, int(with_probs), int(slot), C.byref(p), C.byref(nb), C.byref(nr)))
        _check(lib().gs_match_get_device(self.h, C.byref(d)))
        return _fetch_device(d.value, p, nb.value), nr.value

    def compact_records(self, with_probs=False, slot=0):
        """gs_match_compact_records: the same for the last FASTA or general FASTQ chunk -> (bytes as numpy uint8, records)"""
        p, nb, nr, d = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int(0)
        _check(lib().gs_match_compact_records(self.h, int(with_probs), int(slot), C.byref(p), C.byref(nb), C.byref(nr)))
        _check(lib().gs_match_get_device(self.h, C.byref(d)))
        return _fetch_device(d.value, p, nb.value), nr.value

    def set_taxids(self, taxids):
        """gs_match_set_taxids: the taxid string of every value index (str or bytes), for kraken_text; may be called again"""
        raw = [t.encode() if isinstance(t, str) else bytes(t) for t in taxids]
        assert len(raw) == self.store.n_values, "one taxid string per value index"
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        _check(lib().gs_match_set_taxids(self.h, arr))

    def kraken_text(self, write_all=True, slot=0):
        """gs_match_kraken_text: the Kraken-style lines of the last four-line chunk (submitted with a class array), written on the
        device -> bytes.  To be called before the next submit; segments_fetch-style calls see this chunk's segments afterwards."""
        p, nb, nl, d = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int(0)
        _check(lib().gs_match_kraken_text(self.h, int(bool(write_all)), int(slot), C.byref(p), C.byref(nb), C.byref(nl)))
        _check(lib().gs_match_get_device(self.h, C.byref(d)))
        self.kraken_lines = nl.value
        return _fetch_device(d.value, p, nb.value).tobytes()

    def kraken_records(self, write_all=True, slot=0):
        """gs_match_kraken_records: the same for the last FASTA or general FASTQ chunk -> bytes"""
        p, nb, nl, d = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int(0)
        _check(lib().gs_match_kraken_records(self.h, int(bool(write_all)), int(slot), C.byref(p), C.byref(nb), C.byref(nl)))
        _check(lib().gs_match_get_device(self.h, C.byref(d)))
        self.kraken_lines = nl.value
        return _fetch_device(d.value, p, nb.value).tobytes()

    def text_segments(self):
        """Kraken-style segments of the last text chunk (gs_match_segments_text + gs_match_segments_fetch):
        (seg_off uint64[n + 1], codes int32[], starts int32[])"""
        seg_off = np.zeros(int(self._text_reads) + 1, dtype=np.uint64)
        _check(lib().gs_match_segments_text(self.h, seg_off.ctypes.data_as(C.c_void_p)))
        codes, starts = self.segments_fetch(int(seg_off[-1]))
        return seg_off, codes, starts

    def segments_fetch(self, total):
        """gs_match_segments_fetch alone: (codes, starts) of the `total` segments the last segments call -- or kraken_text, which
        computes them -- has left on the device"""
        codes = np.zeros(max(int(total), 1), dtype=np.int32)
        starts = np.zeros(max(int(total), 1), dtype=np.int32)
        _check(lib().gs_match_segments_fetch(self.h, codes.ctypes.data_as(C.c_void_p), starts.ctypes.data_as(C.c_void_p)))
        return codes[:int(total)], starts[:int(total)]

    def kraken_time(self):
        """gs_match_kraken_time: (event pairs, device ms) of the text kernels of kraken_text so far -- a pair around the size pass and
        one around the write pass of every call (MatchConfig(profile=True))"""
        n, ms = C.c_int64(0), C.c_double(0.0)
        _check(lib().gs_match_kraken_time(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def text_wait_copy(self, ticket):
        _check(lib().gs_match_text_wait_copy(self.h, ticket))

    def text_status(self):
        """(failed_ticket or -1, first_bad_record or -1, (reads, kmers, bases) accepted so far); synchronises"""
        ft, fb = C.c_int64(-1), C.c_int64(-1)
        tot = (C.c_int64 * 3)()
        _check(lib().gs_match_text_status(self.h, C.byref(ft), C.byref(fb), tot))
        return ft.value, fb.value, tuple(tot)

    def text_clear_error(self):
        _check(lib().gs_match_text_clear_error(self.h))

    def text_select(self, bank):
        """chunks of files that are read side by side go to different banks (independent refusal state and totals)"""
        _check(lib().gs_match_text_select(self.h, bank))

    def sync(self):
        _check(lib().gs_match_sync(self.h))

    # ---- DB-partitioned mode (device tensors with data_ptr())
    def encode(self, seq, offsets, pos_off, keys, n_reads):
        _ready(seq, offsets, pos_off, keys)
        _check(lib().gs_match_encode(self.h, C.c_void_p(seq.data_ptr()), C.c_void_p(offsets.data_ptr()), n_reads,
                                     C.c_void_p(pos_off.data_ptr()), C.c_void_p(keys.data_ptr())))

    def probe_keys(self, keys, nodes, n_keys):
        _ready(keys, nodes)
        _check(lib().gs_match_probe_keys(self.h, C.c_void_p(keys.data_ptr()), n_keys, C.c_void_p(nodes.data_ptr())))

    def encode_route(self, seq, offsets, pos_off, n_reads, n_parts, cap, send_keys, send_idx, nodes):
        """gs_match_encode_route: returns (per-owner slot counts, overflow flag)"""
        counts = (C.c_int64 * n_parts)()
        over = C.c_int(0)
        _ready(seq, offsets, pos_off, send_keys, send_idx, nodes)
        _check(lib().gs_match_encode_route(self.h, C.c_void_p(seq.data_ptr()), C.c_void_p(offsets.data_ptr()), n_reads,
                                           C.c_void_p(pos_off.data_ptr()), n_parts, cap, C.c_void_p(send_keys.data_ptr()),
                                           C.c_void_p(send_idx.data_ptr()), C.c_void_p(nodes.data_ptr()), counts, C.byref(over)))
        return list(counts), bool(over.value)

    def route_geometry(self, n_reads):
        """gs_match_route_geometry: (waves gs_match_encode_route launches for n_reads reads, slots per chunk)"""
        w, c = C.c_int32(0), C.c_int32(0)
        _check(lib().gs_match_route_geometry(self.h, n_reads, C.byref(w), C.byref(c)))
        return int(w.value), int(c.value)

    def unroute_region(self, idx, back, n, nodes):
        _ready(idx, back, nodes)
        _check(lib().gs_unroute_region(self.h, C.c_void_p(idx.data_ptr()), C.c_void_p(back.data_ptr()), n, C.c_void_p(nodes.data_ptr())))

    def route_keys(self, keys, n_keys, n_parts, send_keys, idx, nodes=None):
        """device counting sort of the valid keys by owner rank; returns the per-owner counts (python list).
        nodes (int32 tensor, optional): the unrouted positions get their node (miss / invalid) here already"""
        counts = (C.c_int64 * n_parts)()
        _ready(keys, send_keys, idx, nodes)
        _check(lib().gs_route_keys(self.h, C.c_void_p(keys.data_ptr()), n_keys, n_parts, C.c_void_p(send_keys.data_ptr()),
                                   C.c_void_p(idx.data_ptr()), counts, None if nodes is None else C.c_void_p(nodes.data_ptr())))
        return list(counts)

    def unroute_nodes(self, keys, idx, back, n_routed, nodes, n_keys):
        """keys = None: route_keys(..., nodes) has written the unrouted positions already"""
        _ready(keys, idx, back, nodes)
        _check(lib().gs_unroute_nodes(self.h, None if keys is None else C.c_void_p(keys.data_ptr()), C.c_void_p(idx.data_ptr()),
                                      C.c_void_p(back.data_ptr()), n_routed, C.c_void_p(nodes.data_ptr()), n_keys))

    def reduce(self, seq, offsets, pos_off, nodes, n_reads, first_read_no=0, class_vi=None, flags=None):
        _ready(seq, offsets, pos_off, nodes, class_vi, flags)
        _check(lib().gs_match_reduce(self.h, C.c_void_p(seq.data_ptr()), C.c_void_p(offsets.data_ptr()), n_reads,
                                     first_read_no, C.c_void_p(pos_off.data_ptr()), C.c_void_p(nodes.data_ptr()),
                                     None if class_vi is None else C.c_void_p(class_vi.data_ptr()),
                                     None if flags is None else C.c_void_p(flags.data_ptr())))

    def segments(self, seq, offsets):
        """Kraken-style segments of a host batch: (seg_off uint64[n+1], codes int32[], starts int32[], lens int32[])"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        if len(seq) == 0:
            seq = np.zeros(1, dtype=np.uint8)
        seg_off = np.zeros(n + 1, dtype=np.uint64)
        _check(lib().gs_match_segments(self.h, seq.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), n,
                                       MEM_HOST, seg_off.ctypes.data_as(C.c_void_p)))
        total = int(seg_off[-1])
        codes = np.zeros(total, dtype=np.int32)
        starts = np.zeros(total, dtype=np.int32)
        _check(lib().gs_match_segments_fetch(self.h, codes.ctypes.data_as(C.c_void_p), starts.ctypes.data_as(C.c_void_p)))
        # a run ends where the next run of the same read starts, the last one at L - k + 1
        lens = np.zeros(total, dtype=np.int32)
        if total:
            nxt = np.empty(total, dtype=np.int64)
            nxt[:-1] = starts[1:]
            last = seg_off[1:][seg_off[1:] > seg_off[:-1]].astype(np.int64) - 1
            rl = (offsets[1:] - offsets[:-1]).astype(np.int64)[seg_off[1:] > seg_off[:-1]]
            nxt[last] = rl - self.store.k + 1
            lens = (nxt - starts).astype(np.int32)
        return seg_off, codes, starts, lens

    def finish(self):
        nv = self.store.n_values
        t = np.zeros((nv, N_COLS), dtype=np.int64)
        d = np.zeros((nv, N_DCOLS), dtype=np.float64)
        _check(lib().gs_match_finish(self.h, t.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)))
        return t, d

    def max_counts(self):
        """(n_values + 1) x max_kmer_res_counts int16: largest per-k-mer hit counts per value index, last row = total"""
        n = self.config.max_kmer_res_counts
        out = np.zeros((self.store.n_values + 1, max(n, 1)), dtype=np.int16)
        _check(lib().gs_match_max_counts(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def reset(self):
        _check(lib().gs_match_reset(self.h))

    def max_contig_reads(self):
        """per value index: the read number that holds the longest contig so far (-1: none); synchronises"""
        out = np.zeros(self.store.n_values, dtype=np.int64)
        _check(lib().gs_match_max_contig_reads(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def device_state(self):
        """raw device pointers of the accumulators: dict(sums, max_keys, dsums, bitmap, bitmap_words)"""
        s, m, d, b = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        w = C.c_int64(0)
        _check(lib().gs_match_device_state(self.h, C.byref(s), C.byref(m), C.byref(d), C.byref(b), C.byref(w)))
        return dict(sums=s.value, max_keys=m.value, dsums=d.value, bitmap=b.value, bitmap_words=w.value)

    def or_bitmap(self, parts_ptr, n_parts):
        _check(lib().gs_match_or_bitmap(self.h, C.c_void_p(parts_ptr), n_parts))

    def kernel_time(self):
        n, ms = C.c_int64(0), C.c_double(0)
        _check(lib().gs_match_kernel_time(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def prefilter_info(self):
        """The sampled 15-mer prefilter of fixed-length batches: {"built": the store holds a filter, "n_lmers": distinct canonical
        15-mers of the store (-1: never counted), "survivors", "reads": of the last submitted batch (survivors -1: the batch went
        without the prefilter)}.  Synchronises."""
        info = (C.c_int64 * 4)()
        _check(lib().gs_match_prefilter_info(self.h, info))
        return {"built": bool(info[0]), "n_lmers": int(info[1]), "survivors": int(info[2]), "reads": int(info[3])}

    def sn_info(self):
        """Reads that left the match kernel as records (fixed-length batches, counters in LDS): {"deferred": the last submitted
        batch ran that way, "booked": the records of reads of one tax id the reduce kernel booked for it, "rows": the reads that
        left as the node of every position (several tax ids, or a non-CGAT byte)}.  Synchronises."""
        info = (C.c_int64 * 3)()
        _check(lib().gs_match_sn_info(self.h, info))
        return {"deferred": bool(info[0]), "booked": int(info[1]), "rows": int(info[2])}

    def gate_info(self):
        """Reads behind the prefilter skip the minimizer gate: {"gateless": the last submitted batch ran without the gate,
        "predicted_pass": the pass probability of a random read the rule used for it (-1: the batch could not go that way)}."""
        g, p = C.c_int(0), C.c_double(0)
        _check(lib().gs_match_gate_info(self.h, C.byref(g), C.byref(p)))
        return {"gateless": bool(g.value), "predicted_pass": p.value}

    def close(self):
        if getattr(self, "h", None):
            lib().gs_match_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BloomInfo(C.Structure):
    """gs_bloom_info: k = 0, expected_insertions / n_inserted = -1 and fpp = 0 stand for "unknown" """
    _fields_ = [("kind", C.c_int32), ("k", C.c_int32), ("n_hashes", C.c_int32), ("pad", C.c_int32), ("bits", C.c_int64),
                ("n_words", C.c_int64), ("expected_insertions", C.c_int64), ("n_inserted", C.c_int64), ("fpp", C.c_double)]


def requested_mask(taxids, requested_taxids):
    """uint8[len(taxids)] for DeviceBloomFilter.from_store: 1 where the value's tax id (taxids[value index], strings) is one of
    `requested_taxids`.  A requested tax id the store does not know is an error, as a mistyped one would build an empty index."""
    want = {str(t) for t in requested_taxids}
    unknown = want - {str(t) for t in taxids}
    if unknown:
        raise ValueError(f"tax ids not in the store: {sorted(unknown)}")
    return np.array([str(t) in want for t in taxids], dtype=np.uint8)


class DeviceBloomFilter:
    """device copy of a reference index filter (bits + hash factors replicated exactly)."""

    def __init__(self, kind, bits, hash_factors, words, n_hashes=None, device=0):
        hf = np.ascontiguousarray(hash_factors, dtype=np.int64)
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if n_hashes is None:
            n_hashes = len(hf)
        self.h = C.c_void_p()
        _check(lib().gs_bloom_create(C.byref(self.h), device, kind, bits, n_hashes, hf.ctypes.data_as(C.c_void_p),
                                     w.ctypes.data_as(C.c_void_p), len(w)))

    @classmethod
    def build(cls, kmers, expected_insertions=None, fpp=1e-8, device=0, kind=BLOOM_XOR):
        """gs_bloom_build: the XOR (or Murmur) index filter over `kmers` (numpy int64 or a device tensor), sized like the
        reference's (BloomIndexGoal: indexBloomFilterFpp, default 1e-8) and filled on the device"""
        pk, mem = _ptr(kmers)
        n = int(kmers.shape[0] if hasattr(kmers, "shape") else len(kmers))
        _ready(kmers)
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        _check(lib().gs_bloom_build(C.byref(self.h), device, kind, pk, n, mem, int(expected_insertions or max(n, 1)), float(fpp)))
        return self

    @classmethod
    def from_store(cls, store, requested, kind=BLOOM_XOR, fpp=1e-8, expected_insertions=None):
        """gs_bloom_build_db, the index goal (BloomIndexGoal): the filter of `kind` over the stored k-mers of `store` whose value
        is requested (bool / uint8 [n_values], the per-node flag: see requested_mask), sized for their count (or for
        expected_insertions) like the reference's and filled on the device.  The count is info().n_inserted."""
        req = np.ascontiguousarray(np.asarray(requested) != 0, dtype=np.uint8)
        if req.ndim != 1 or len(req) != store.info.n_values:
            raise ValueError(f"requested has shape {req.shape}, the store has {store.info.n_values} values")
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        _check(lib().gs_bloom_build_db(C.byref(self.h), store.h, kind, req.ctypes.data_as(C.c_void_p),
                                       -1 if expected_insertions is None else int(expected_insertions), float(fpp), None))
        return self

    @classmethod
    def load(cls, path, device=0):
        """open a native index file written by save() (gs_bloom_load)"""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        _check(lib().gs_bloom_load(C.byref(self.h), device, str(path).encode()))
        return self

    def save(self, path):
        _check(lib().gs_bloom_save(self.h, str(path).encode()))

    def info(self):
        i = BloomInfo()
        _check(lib().gs_bloom_get_info(self.h, C.byref(i)))
        return i

    @property
    def device(self):
        d = C.c_int(0)
        _check(lib().gs_filter_get_device(self.h, C.byref(d)))
        return d.value

    def get(self, with_words=True):
        """-> (bits, hash_factors int64[], words uint64[] or None)"""
        bits, nh = C.c_int64(0), C.c_int32(0)
        _check(lib().gs_bloom_get(self.h, C.byref(bits), C.byref(nh), None, None, 0))
        hf = np.zeros(nh.value, dtype=np.int64)
        words = np.zeros(self.info().n_words, dtype=np.uint64) if with_words else None
        _check(lib().gs_bloom_get(self.h, None, None, hf.ctypes.data_as(C.c_void_p),
                                  None if words is None else words.ctypes.data_as(C.c_void_p), 0 if words is None else len(words)))
        return bits.value, hf, words

    def close(self):
        if getattr(self, "h", None):
            lib().gs_bloom_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FastqBloomFilter:
    def __init__(self, k, bloom, min_pos_count=1, positive_ratio=0.2, profile=False):
        self.k, self.bloom, self.min_pos_count, self.positive_ratio = k, bloom, min_pos_count, positive_ratio
        self.profile = profile

    def submit(self, seq, offsets, accept, n_reads=None):
        ps, mem = _ptr(seq)
        po, _ = _ptr(offsets)
        pa, _ = _ptr(accept)
        if n_reads is None:
            n_reads = (offsets.shape[0] if hasattr(offsets, "shape") else len(offsets)) - 1
        _ready(seq, offsets, accept)
        _check(lib().gs_filter_submit(self.bloom.h, self.k, self.min_pos_count, self.positive_ratio, ps, po, n_reads,
                                      mem, pa, int(self.profile)))

    def submit_text(self, text, accept, n_lines=None, newlines=None):
        """raw FASTQ text of whole 4-line records (gs_filter_submit_text); returns the ticket"""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        if n_lines is None:
            n_lines = int((text == 10).sum())
        n_bytes = int(text.shape[0])
        pt, mem = _ptr(text) if n_bytes else (None, MEM_HOST)
        pa, _ = _ptr(accept)
        pn, _ = _ptr(newlines)
        _ready(text, accept, newlines)
        ticket = C.c_int64(-1)
        self._text_keep = text
        _check(lib().gs_filter_submit_text(self.bloom.h, self.k, self.min_pos_count, self.positive_ratio, pt, n_bytes,
                                           int(n_lines), mem, pa, pn, int(self.profile), C.byref(ticket)))
        return ticket.value

    def submit_fasta(self, text, accept, n_records=None, n_lines=None):
        """raw FASTA text of whole records (gs_filter_submit_fasta): accept[r] per record; -> read lengths"""
        text = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        if n_lines is None:
            n_lines = int((text == 10).sum())
        if n_records is None:
            t = np.asarray(text)
            n_records = int(np.count_nonzero((t == 62) & np.concatenate(([True], t[:-1] == 10))))
        ticket = C.c_int64(-1)
        self._text_keep = text
        _check(lib().gs_filter_submit_fasta(self.bloom.h, self.k, self.min_pos_count, self.positive_ratio, _ptr(text)[0], int(text.shape[0]),
                                            int(n_lines), int(n_records), MEM_HOST, _ptr(accept)[0], None, C.byref(ticket)))
        return self._read_lengths(n_records)

    def submit_fastq_ml(self, text, accept, n_lines=None):
        """general FASTQ text starting at a descriptor line (gs_filter_submit_fastq_ml): -> (records filtered or -1 when refused,
        bytes they cover, read lengths)"""
        text = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text
        if n_lines is None:
            n_lines = int((text == 10).sum())
        n_rec, used, ticket = C.c_int64(0), C.c_int64(0), C.c_int64(-1)
        self._text_keep = text
        _check(lib().gs_filter_submit_fastq_ml(self.bloom.h, self.k, self.min_pos_count, self.positive_ratio, _ptr(text)[0],
                                               int(text.shape[0]), int(n_lines), MEM_HOST, _ptr(accept)[0], None, C.byref(n_rec),
                                               C.byref(used), None, C.byref(ticket)))
        return n_rec.value, used.value, (self._read_lengths(n_rec.value) if n_rec.value > 0 else np.zeros(0, dtype=np.int64))

    def _read_lengths(self, n_records):
        b = np.zeros(n_records + 1, dtype=np.uint64)
        if n_records > 0:
            _check(lib().gs_filter_text_read_bounds(self.bloom.h, _ptr(b)[0]))
        else:
            _check(lib().gs_filter_sync(self.bloom.h))
        return np.diff(b.astype(np.int64))

    def text_status(self):
        ft, fb = C.c_int64(-1), C.c_int64(-1)
        tot = (C.c_int64 * 3)()
        _check(lib().gs_filter_text_status(self.bloom.h, C.byref(ft), C.byref(fb), tot))
        return ft.value, fb.value, tuple(tot)

    def compact_text(self, which=1, with_probs=False, slot=0):
        """gs_filter_compact_text: the accepted (which = 1) / other records of the last four-line chunk as ReadEntry.write writes them,
        gathered on the device -> (bytes as numpy uint8, records)"""
        p, nb, nr = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        _check(lib().gs_filter_compact_text(self.bloom.h, int(which), int(with_probs), int(slot), C.byref(p), C.byref(nb), C.byref(nr)))
        return _fetch_device(self.bloom.device, p, nb.value), nr.value

    def compact_records(self, which=1, with_probs=False, slot=0):
        """gs_filter_compact_records: the same for the last FASTA or general FASTQ chunk -> (bytes as numpy uint8, records)"""
        p, nb, nr = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        _check(lib().gs_filter_compact_records(self.bloom.h, int(which), int(with_probs), int(slot), C.byref(p), C.byref(nb), C.byref(nr)))
        return _fetch_device(self.bloom.device, p, nb.value), nr.value

    def text_reset(self, clear_totals=False):
        _check(lib().gs_filter_text_reset(self.bloom.h, int(clear_totals)))

    def accept_reads(self, seq, offsets):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        acc = np.zeros(len(offsets) - 1, dtype=np.uint8)
        if len(seq) == 0:
            seq = np.zeros(1, dtype=np.uint8)
        self.submit(seq, offsets, acc)
        return acc

    def sync(self):
        _check(lib().gs_filter_sync(self.bloom.h))

    def kernel_time(self):
        n, ms = C.c_int64(0), C.c_double(0)
        _check(lib().gs_filter_kernel_time(self.bloom.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value


def _text_counts(text):
    """(uint8 array, newlines, header lines) of a chunk of text"""
    t = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    if t.shape[0] == 0:
        return np.zeros(1, dtype=np.uint8), 0, 0, 0
    return t, int(t.shape[0]), int((t == 10).sum()), int(np.count_nonzero((t == 62) & np.concatenate(([True], t[:-1] == 10))))


class DeviceReads:
    """gs_reads: the text stage without a store or a filter -- the extract goal's selection by descriptor prefix and the
    fasta2fastq goal's text, both on the device"""

    def __init__(self, device=0, k=31):
        self.h = C.c_void_p()
        self.device, self.k = int(device), int(k)
        _check(lib().gs_reads_create(C.byref(self.h), self.device))

    def close(self):
        if self.h:
            lib().gs_reads_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    @staticmethod
    def _key(key):
        key = bytes(key)
        return np.frombuffer(key, dtype=np.uint8) if key else np.zeros(1, dtype=np.uint8), len(key)

    def select_text(self, text, key):
        """four-line FASTQ text of whole records -> accept flag per record"""
        t, nb, nl, _ = _text_counts(text)
        kb, kl = self._key(key)
        acc = np.zeros(max(nl // 4, 1), dtype=np.uint8)
        _check(lib().gs_reads_select_text(self.h, self.k, _ptr(t)[0], nb, nl, MEM_HOST, _ptr(kb)[0], kl, _ptr(acc)[0], None, None))
        _check(lib().gs_reads_sync(self.h))
        return acc[:nl // 4]

    def select_fasta(self, text, key):
        """FASTA text of whole records -> accept flag per record"""
        t, nb, nl, nr = _text_counts(text)
        kb, kl = self._key(key)
        acc = np.zeros(max(nr, 1), dtype=np.uint8)
        _check(lib().gs_reads_select_fasta(self.h, self.k, _ptr(t)[0], nb, nl, nr, MEM_HOST, _ptr(kb)[0], kl, _ptr(acc)[0], None, None))
        _check(lib().gs_reads_sync(self.h))
        return acc[:nr]

    def select_fastq_ml(self, text, key):
        """general FASTQ text starting at a descriptor line -> (records or -1 when refused, bytes they cover, accept flags)"""
        t, nb, nl, _ = _text_counts(text)
        kb, kl = self._key(key)
        acc = np.zeros(nl // 4 + 2, dtype=np.uint8)
        n_rec, used = C.c_int64(0), C.c_int64(0)
        _check(lib().gs_reads_select_fastq_ml(self.h, self.k, _ptr(t)[0], nb, nl, MEM_HOST, _ptr(kb)[0], kl, _ptr(acc)[0], None, C.byref(n_rec),
                                              C.byref(used), None, None))
        _check(lib().gs_reads_sync(self.h))
        return n_rec.value, used.value, acc[:max(n_rec.value, 0)]

    def compact_text(self, with_probs=True, slot=0):
        """the selected records of the last four-line or FASTA chunk as ReadEntry.write writes them -> (bytes, records)"""
        p, nb, nr = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        _check(lib().gs_reads_compact_text(self.h, int(with_probs), int(slot), C.byref(p), C.byref(nb), C.byref(nr)))
        return _fetch_device(self.device, p, nb.value), nr.value

    def compact_records(self, with_probs=True, slot=0):
        """the selected records of the last FASTA or general FASTQ chunk as ReadEntry.write writes them, the latter with their
        quality lines if with_probs -> (bytes, records)"""
        p, nb, nr = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        _check(lib().gs_reads_compact_records(self.h, int(with_probs), int(slot), C.byref(p), C.byref(nb), C.byref(nr)))
        return _fetch_device(self.device, p, nb.value), nr.value

    def fasta2fastq(self, text, n_lines=None, n_records=None, slot=0):
        """the fasta2fastq goal's text of a FASTA chunk -> (bytes as numpy uint8, lines of 65 534 bytes and more); a refused chunk
        gives no bytes and shows in text_status()"""
        t, nb, nl, nr = _text_counts(text)
        p, n_out, long_lines = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        _check(lib().gs_reads_fasta2fastq(self.h, _ptr(t)[0], nb, nl if n_lines is None else int(n_lines), nr if n_records is None else int(n_records),
                                          MEM_HOST, int(slot), C.byref(p), C.byref(n_out), C.byref(long_lines), None))
        return _fetch_device(self.device, p, n_out.value), long_lines.value

    def text_status(self):
        ft, fb = C.c_int64(-1), C.c_int64(-1)
        tot = (C.c_int64 * 3)()
        _check(lib().gs_reads_text_status(self.h, C.byref(ft), C.byref(fb), tot))
        return ft.value, fb.value, tuple(tot)

    def text_reset(self, clear_totals=False):
        _check(lib().gs_reads_text_reset(self.h, int(clear_totals)))

    def kernel_time(self, profile=True):
        """(launches, milliseconds) of the FASTA -> FASTQ text kernels so far; switches their timing on or off"""
        n, ms = C.c_int64(0), C.c_double(0)
        _check(lib().gs_reads_kernel_time(self.h, int(profile), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def phase_times(self):
        """{phase: (launches, milliseconds)} of a profiling handle so far: "select" (a chunk from its submission to its flags),
        "gather" (the four-line gather of compact_text), "rewrite" (the FASTA -> FASTQ text kernels, as kernel_time)"""
        n, ms = (C.c_int64 * 3)(), (C.c_double * 3)()
        _check(lib().gs_reads_phase_times(self.h, n, ms))
        return {name: (n[i], ms[i]) for i, name in enumerate(("select", "gather", "rewrite"))}


class KrakenCounter:
    """gs_krakencount: Kraken-style output lines counted per tax id on the device (the krakencount goal).  A chunk outside the
    device's grammar is refused and adds nothing: genestrip_amd.host.kraken_count_files hands such chunks to the reference-exact
    parser; here the caller sees the refusal in the chunk's report."""

    def __init__(self, device=0, max_taxids=1 << 16):
        self.h = C.c_void_p()
        self.device = int(device)
        _check(lib().gs_krakencount_create(C.byref(self.h), self.device, int(max_taxids)))

    def close(self):
        if self.h:
            lib().gs_krakencount_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def geometry(self):
        g = (C.c_int64 * 6)()
        _check(lib().gs_krakencount_geometry(self.h, g))
        return {"tile_bytes": g[0], "lds_slots": g[1], "global_slots": g[2], "scan_levels": g[3], "scan_block_bytes": g[4],
                "level3_blocks": g[5]}

    def submit(self, text):
        """a chunk of whole lines (bytes, a uint8 array, or a uint8 tensor on the handle's device) -> its ticket"""
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        _ready(text)
        p, mem = _ptr(text) if n else (None, MEM_HOST)
        ticket = C.c_int64()
        _check(lib().gs_krakencount_submit(self.h, p, n, mem, C.byref(ticket)))
        return ticket.value

    def chunk(self, ticket):
        """what became of a chunk: refused (0 counted, 1 outside the grammar, 2 table full), its first bad line, the offset of its
        first empty line (-1: none), the table's rows behind it, its own totals"""
        r = (C.c_int64 * 8)()
        _check(lib().gs_krakencount_chunk(self.h, int(ticket), r))
        return {"refused": r[0], "first_bad_line": r[1], "first_empty_offset": r[2], "rows": r[3], "totals": tuple(r[4:8])}

    def status(self):
        """(first refused ticket or -1, its first bad line, first-empty-line offset of the latest chunk, totals = lines, counted
        tokens, skipped 'A' tokens, long lines)"""
        ft, fb, fe = C.c_int64(), C.c_int64(), C.c_int64()
        tot = (C.c_int64 * 4)()
        _check(lib().gs_krakencount_status(self.h, C.byref(ft), C.byref(fb), C.byref(fe), tot))
        return ft.value, fb.value, fe.value, tuple(tot)

    def reset(self):
        _check(lib().gs_krakencount_reset(self.h))

    def fetch(self):
        """(taxids int32[n], counts int64[n, 3] = reads, kmers, kmers in matching reads), rows in the reference's order"""
        n = C.c_int64()
        _check(lib().gs_krakencount_fetch(self.h, None, None, 0, C.byref(n)))
        ids = np.zeros(max(n.value, 1), dtype=np.int32)
        cnt = np.zeros((max(n.value, 1), 3), dtype=np.int64)
        _check(lib().gs_krakencount_fetch(self.h, _ptr(ids)[0], _ptr(cnt)[0], n.value, C.byref(n)))
        return ids[:n.value], cnt[:n.value]

    def counters(self):
        """(global atomics issued by the accumulation, tokens whose key found no room in a workgroup's table)"""
        c = (C.c_int64 * 2)()
        _check(lib().gs_krakencount_counters(self.h, c))
        return c[0], c[1]

    def kernel_time(self, profile=True):
        n, ms = C.c_int64(), C.c_double()
        _check(lib().gs_krakencount_kernel_time(self.h, int(profile), C.byref(n), C.byref(ms)))
        return n.value, ms.value


class _AccmapCfg(C.Structure):
    _fields_ = [("dna", C.c_int32), ("rna", C.c_int32), ("mrna", C.c_int32), ("n_categories", C.c_int32), ("n_statuses", C.c_int32),
                ("n_nodes", C.c_int32), ("categories", C.POINTER(C.c_char_p)), ("statuses", C.POINTER(C.c_char_p)),
                ("known_taxids", C.c_void_p), ("reserve_entries", C.c_int64)]


def accession_slots(keys):
    """accessions (bytes, at most 31 each, all below 0x80) -> their 32-byte slots as uint8[n, 32]: length, bytes, zeros"""
    out = np.zeros((len(keys), 32), dtype=np.uint8)
    for i, k in enumerate(keys):
        if len(k) > 31:
            raise ValueError("an accession slot holds at most 31 bytes")
        out[i, 0] = len(k)
        out[i, 1:1 + len(k)] = np.frombuffer(bytes(k), dtype=np.uint8)
    return out


def slot_accessions(slots):
    """uint8[n, 32] slots -> list of accessions (bytes)"""
    return [bytes(s[1:1 + int(s[0])]) for s in np.asarray(slots, dtype=np.uint8).reshape(-1, 32)]


class DeviceAccessionMap:
    """gs_accmap: the lines of a RefSeq catalog to the accession map on the device (the accmapsize and accmap goals).  A node is an
    index into known_taxids (ascending, distinct, positive), -1 is none.  submit() takes chunks of whole lines; a chunk outside the
    device's grammar is refused and leaves the map as it was: the caller parses it and hands its entries in through append().
    Among equal accessions a lookup answers with the one that came first in the input."""

    SEQ_TYPES = {"GENOMIC": (1, 0, 0), "RNA": (0, 1, 0), "M_RNA": (0, 0, 1), "ALL_RNA": (0, 1, 1), "ALL": (1, 1, 1)}

    @classmethod
    def config(cls, known_taxids, categories, statuses, seq_type="GENOMIC", reserve_entries=0):
        """-> (gs_accmap_cfg, known_taxids as int32): the structure keeps the arrays it points to alive"""
        known = np.ascontiguousarray(known_taxids, dtype=np.int32)
        dna, rna, mrna = cls.SEQ_TYPES[seq_type] if isinstance(seq_type, str) else seq_type
        cats = [c.encode() if isinstance(c, str) else bytes(c) for c in categories]
        stats = [s.encode() if isinstance(s, str) else bytes(s) for s in statuses]
        cfg = _AccmapCfg(int(bool(dna)), int(bool(rna)), int(bool(mrna)), len(cats), len(stats), len(known),
                         (C.c_char_p * max(len(cats), 1))(*cats), (C.c_char_p * max(len(stats), 1))(*stats),
                         known.ctypes.data_as(C.c_void_p) if len(known) else None, int(reserve_entries))
        cfg._known = known
        return cfg, known

    def __init__(self, known_taxids, categories, statuses, seq_type="GENOMIC", device=0, reserve_entries=0):
        """seq_type: one of SEQ_TYPES or a (dna, rna, mrna) triple; categories / statuses: strings searched for as substrings;
        device -1: a host-only map (append, finish, fetch and lookups of host memory; no device is touched)"""
        self.h = C.c_void_p()
        self.device = int(device)
        cfg, self.known = self.config(known_taxids, categories, statuses, seq_type, reserve_entries)
        self.n_entries = self.n_passing = self.n_duplicates = self.n_conflicts = 0
        _check(lib().gs_accmap_create(C.byref(self.h), self.device, C.byref(cfg)))

    @classmethod
    def _wrap(cls, handle, known_taxids):
        """a finished map that the host layer made (host.accmap_files); its device is -1 if it is a host-only one"""
        m = cls.__new__(cls)
        m.h = handle
        m.known = np.ascontiguousarray(known_taxids, dtype=np.int32)
        dev = C.c_int(0)
        _check(lib().gs_accmap_get_device(m.h, C.byref(dev)))
        m.device = dev.value
        m.n_entries = m.n_passing = m.n_duplicates = m.n_conflicts = 0
        return m

    def close(self):
        if getattr(self, "h", None):
            lib().gs_accmap_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def submit(self, text, last=False):
        """a chunk of whole lines (bytes, a uint8 array, or a uint8 tensor on the handle's device); last: the stream ends here and
        its final line need not be terminated -> its report"""
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        _ready(text)
        p, mem = _ptr(text) if n else (None, MEM_HOST)
        r = (C.c_int64 * 8)()
        _check(lib().gs_accmap_submit(self.h, p, n, mem, int(bool(last)), r))
        return {"lines": r[0], "passing": r[1], "put": r[2], "refused": r[3], "first_bad_line": r[4], "longest_line": r[5]}

    def append(self, keys, nodes, n_passing=None):
        """entries made elsewhere, in input order: keys (accessions as bytes, or uint8[n, 32] slots), nodes; n_passing: the passing
        entries of the same lines, those without a node included (default: len(keys))"""
        slots = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 32) if isinstance(keys, np.ndarray) else accession_slots(keys)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        if len(nodes) != len(slots):
            raise ValueError("one node per key")
        n = len(slots)
        _check(lib().gs_accmap_append(self.h, _ptr(slots)[0] if n else None, _ptr(nodes)[0] if n else None, n, n if n_passing is None else int(n_passing)))

    def finish(self):
        """sorts -> (entries, passing entries in all = the accmapsize count, duplicates, conflicts)"""
        info = (C.c_int64 * 4)()
        _check(lib().gs_accmap_finish(self.h, info))
        self.n_entries, self.n_passing, self.n_duplicates, self.n_conflicts = tuple(info)
        return tuple(info)

    def fetch(self):
        """-> (slots uint8[entries, 32] in the map's order, nodes int32[entries], regions int32[n_nodes])"""
        slots = np.zeros((max(self.n_entries, 1), 32), dtype=np.uint8)
        nodes = np.zeros(max(self.n_entries, 1), dtype=np.int32)
        regions = np.zeros(max(len(self.known), 1), dtype=np.int32)
        _check(lib().gs_accmap_fetch(self.h, _ptr(slots)[0], _ptr(nodes)[0], _ptr(regions)[0]))
        return slots[:self.n_entries], nodes[:self.n_entries], regions[:len(self.known)]

    def lookup(self, headers, header_off=None, complete_only=False):
        """headers: a list of header lines (bytes), or the lines back to back (uint8 array or device tensor) with header_off
        (uint64[n + 1], in the same memory) -> node per line: int32 array, or a device tensor if the input was one"""
        if header_off is None:
            lens = np.array([len(x) for x in headers], dtype=np.uint64)
            header_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
            headers = np.frombuffer(b"".join(bytes(x) for x in headers) or b"\0", dtype=np.uint8)
        n = int(header_off.shape[0]) - 1
        _ready(headers, header_off)
        (ph, mem), (po, mem_off) = _ptr(headers), _ptr(header_off)
        if mem != mem_off:
            raise ValueError("headers and header_off must live in the same memory")
        if mem == MEM_DEVICE:
            import torch
            out = torch.empty(max(n, 1), dtype=torch.int32, device=headers.device)
        else:
            out = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().gs_accmap_lookup(self.h, ph, po, n, mem, int(bool(complete_only)), _ptr(out)[0]))
        return out[:n]

    def lookup_genomes(self, genomes, complete_only=False):
        """the header lines of the chunk a DeviceGenomes has scanned, looked up where they are -> node per record (int32)"""
        out = np.zeros(max(genomes.n_records, 1), dtype=np.int32)
        _check(lib().gs_accmap_lookup_genomes(self.h, genomes.h, int(bool(complete_only)), _ptr(out)[0]))
        return out[:genomes.n_records]

    def kernel_time(self, profile=True):
        """(launches, milliseconds) of the scan, finish and lookup kernels so far; switches their timing on or off"""
        n, ms = C.c_int64(), C.c_double()
        _check(lib().gs_accmap_kernel_time(self.h, int(profile), C.byref(n), C.byref(ms)))
        return n.value, ms.value


class _AsmsumCfg(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("known_taxids", C.c_void_p), ("filter", C.c_void_p), ("quality_mask", C.c_int32),
                ("reference_only", C.c_int32), ("use_species_taxid", C.c_int32), ("reserve_entries", C.c_int64)]


ASSEMBLY_QUALITIES = ("ADDITIONAL", "COMPLETE_LATEST", "COMPLETE", "CHROMOSOME_LATEST", "CHROMOSOME", "SCAFFOLD_LATEST", "SCAFFOLD",
                      "CONTIG_LATEST", "CONTIG", "LATEST", "NONE")


def quality_mask(qualities):
    """a list of AssemblyQuality names or ordinals -> the mask of gs_asmsum_cfg; None (the reference's null list) -> -1: all"""
    if qualities is None:
        return -1
    mask = 0
    for q in qualities:
        mask |= 1 << (ASSEMBLY_QUALITIES.index(q) if isinstance(q, str) else int(q))
    return mask


def file_name_of(ftp):
    """gs_asmsum_file_name: AssemblyEntry's file name of an ftp path (bytes or str) -> bytes"""
    ftp = ftp.encode() if isinstance(ftp, str) else bytes(ftp)
    out = np.zeros(len(ftp) + 16, dtype=np.uint8)
    n = lib().gs_asmsum_file_name(ftp, len(ftp), out.ctypes.data_as(C.c_void_p), len(out))
    if n < 0:
        _check(int(n))
    return out[:n].tobytes()


class DeviceAssemblySummary:
    """gs_asmsum: the lines of a Genbank assembly summary to the picks per tree node on the device (the fastasgenbank goal).  A node is
    an index into known_taxids (ascending, distinct, positive).  submit() takes chunks of whole lines; a chunk outside the device's
    grammar is refused and leaves the handle as it was: the caller parses it and hands its entries in through append().  finish()
    applies the cap; fetch() gives the picked entries, nodes ascending."""

    @classmethod
    def config(cls, known_taxids, filter=None, qualities=("COMPLETE_LATEST", "CHROMOSOME_LATEST"), reference_only=False, use_species_taxid=False,
               reserve_entries=0):
        """-> gs_asmsum_cfg; the structure keeps the arrays it points to alive.  filter: node flags (uint8[n_nodes]) or None"""
        known = np.ascontiguousarray(known_taxids, dtype=np.int32)
        flt = None if filter is None else np.ascontiguousarray(filter, dtype=np.uint8)
        if flt is not None and len(flt) != len(known):
            raise ValueError("one filter flag per node")
        cfg = _AsmsumCfg(len(known), known.ctypes.data_as(C.c_void_p) if len(known) else None,
                         flt.ctypes.data_as(C.c_void_p) if flt is not None and len(flt) else None, quality_mask(qualities),
                         int(bool(reference_only)), int(bool(use_species_taxid)), int(reserve_entries))
        cfg._keep = (known, flt)
        return cfg

    def __init__(self, known_taxids, filter=None, qualities=("COMPLETE_LATEST", "CHROMOSOME_LATEST"), reference_only=False,
                 use_species_taxid=False, device=0, reserve_entries=0):
        """device -1: a host-only handle (append, finish, fetch; no device is touched)"""
        self.h = C.c_void_p()
        self.device = int(device)
        self.info = None
        cfg = self.config(known_taxids, filter, qualities, reference_only, use_species_taxid, reserve_entries)
        _check(lib().gs_asmsum_create(C.byref(self.h), self.device, C.byref(cfg)))

    @classmethod
    def _wrap(cls, handle, info=None):
        """a finished handle that the host layer made (host.assembly_summary_files)"""
        m = cls.__new__(cls)
        m.h = handle
        dev = C.c_int(0)
        _check(lib().gs_asmsum_get_device(m.h, C.byref(dev)))
        m.device = dev.value
        m.info = info
        return m

    def close(self):
        if getattr(self, "h", None):
            lib().gs_asmsum_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def submit(self, text, last=False):
        """a chunk of whole lines (bytes, a uint8 array, or a uint8 tensor on the handle's device); last: the stream ends here and
        its final line need not be terminated -> its report"""
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        n = int(text.shape[0])
        _ready(text)
        p, mem = _ptr(text) if n else (None, MEM_HOST)
        r = (C.c_int64 * 8)()
        _check(lib().gs_asmsum_submit(self.h, p, n, mem, int(bool(last)), r))
        return {"counted": r[0], "kept": r[1], "short": r[2], "refused": r[3], "first_bad_line": r[4], "longest_line": r[5], "skipped": r[6],
                "pool_bytes": r[7]}

    def append(self, entries, n_counted=None, n_lines=None):
        """entries made elsewhere, in input order: (node, taxid, species_taxid, ftp, quality, is_ref, line) each, the three strings as
        bytes; n_counted: the counted records of the same lines (default: len(entries)); n_lines: those lines (default: n_counted)"""
        n = len(entries)
        nodes = np.array([e[0] for e in entries], dtype=np.int32)
        quality = np.array([e[4] for e in entries], dtype=np.uint8)
        is_ref = np.array([bool(e[5]) for e in entries], dtype=np.uint8)
        lines = np.array([e[6] for e in entries], dtype=np.int64)
        strs = [bytes(s) for e in entries for s in (e[1], e[2], e[3])]
        off = np.concatenate([np.zeros(1, np.uint64), np.cumsum([len(s) for s in strs], dtype=np.uint64)]).astype(np.uint64)
        pool = np.frombuffer(b"".join(strs) + b"\0", dtype=np.uint8)
        n_counted = n if n_counted is None else int(n_counted)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _check(lib().gs_asmsum_append(self.h, vp(nodes), vp(quality), vp(is_ref), vp(lines), vp(off), vp(pool), n, n_counted,
                                      n_counted if n_lines is None else int(n_lines)))

    def finish(self, max_per_node=1):
        """the cap -> (kept entries, picked entries, nodes with entries, counted records in all)"""
        info = (C.c_int64 * 4)()
        _check(lib().gs_asmsum_finish(self.h, int(max_per_node), info))
        self.info = tuple(info)
        return self.info

    def fetch(self):
        """-> the picked entries, nodes ascending, inside a node in the reference's list order:
        [(node, taxid, species_taxid, ftp, quality, is_ref, line)], the three strings as bytes"""
        m = self.info[1] if self.info else 0  # (in front of finish() the library refuses the call)
        nodes = np.zeros(max(m, 1), dtype=np.int32)
        quality = np.zeros(max(m, 1), dtype=np.uint8)
        is_ref = np.zeros(max(m, 1), dtype=np.uint8)
        lines = np.zeros(max(m, 1), dtype=np.int64)
        off = np.zeros(3 * m + 1, dtype=np.uint64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        _check(lib().gs_asmsum_fetch(self.h, vp(nodes), vp(quality), vp(is_ref), vp(lines), vp(off), None))
        pool = np.zeros(max(int(off[3 * m]), 1), dtype=np.uint8)
        _check(lib().gs_asmsum_fetch(self.h, None, None, None, None, None, vp(pool)))
        raw = pool.tobytes()
        s = lambda i: raw[int(off[i]):int(off[i + 1])]  # noqa: E731
        return [(int(nodes[j]), s(3 * j), s(3 * j + 1), s(3 * j + 2), int(quality[j]), bool(is_ref[j]), int(lines[j])) for j in range(m)]

    def kernel_time(self, profile=True):
        """(launches, milliseconds) of the scan and finish kernels so far; switches their timing on or off"""
        n, ms = C.c_int64(), C.c_double()
        _check(lib().gs_asmsum_kernel_time(self.h, int(profile), C.byref(n), C.byref(ms)))
        return n.value, ms.value


RANK_NAMES = ("cellular root", "acellular root", "superkingdom", "domain", "realm", "kingdom", "phylum", "subphylum", "superclass", "class",
              "subclass", "superorder", "order", "suborder", "superfamily", "family", "subfamily", "tribe", "genus", "subgenus",
              "species group", "species", "varietas", "subspecies", "serogroup", "biotype", "strain", "serotype", "genotype", "forma",
              "forma specialis", "isolate", "clade", "no rank", "subkingdom", "section", "REFINED", "DATA", "FILE", "ID")


def read_taxids(text):
    """gs_taxtree_read_taxids: the bytes of a tax id file as TaxIdCollector.readFromFile reads them -> (requested, excluded) tax ids
    as int32 arrays, in file order; a value that is no tax id of 1-9 digits is dropped, as an unknown id is"""
    buf = np.frombuffer(bytes(text) or b"\0", dtype=np.uint8)
    n = len(bytes(text))
    cap = n // 2 + 1
    req, exc = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    n_req, n_exc = C.c_int64(), C.c_int64()
    _check(lib().gs_taxtree_read_taxids(_ptr(buf)[0], n, _ptr(req)[0], C.byref(n_req), _ptr(exc)[0], C.byref(n_exc), cap))
    return req[:n_req.value], exc[:n_exc.value]


class DeviceTaxTree:
    """gs_taxtree: the lines of an NCBI nodes.dmp and names.dmp to the arrays of the tree (the taxtree goal), the taxnodes selection
    and the tree a database carries.  A node is its index in the ascending array of distinct tax ids, so arrays()["taxids"] is the
    known_taxids of DeviceAccessionMap.  submit_nodes() takes chunks of whole lines on the device; a chunk outside the device's
    grammar is refused and leaves the tree as it was: the caller hands it to append_nodes(), which judges it line by line.
    device -1: a host-only tree (append_nodes, finish, and every query from host memory)."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        self.device = int(device)
        self.n_nodes = self.n_reached = self.max_depth = self.n_duplicates = self.on_host = self.n_cycle_nodes = 0
        _check(lib().gs_taxtree_create(C.byref(self.h), self.device))

    @classmethod
    def _wrap(cls, handle, report):
        """a finished tree that the host layer made (host.taxtree_files); its device is -1 if it is a host-only one"""
        t = cls.__new__(cls)
        t.h = handle
        dev = C.c_int(0)
        _check(lib().gs_taxtree_get_device(t.h, C.byref(dev)))
        t.device = dev.value
        t.n_nodes, t.n_reached, t.n_duplicates, t.on_host = report["nodes"], report["reached"], report["duplicates"], report["on_host"]
        t.n_cycle_nodes = 0
        t.max_depth = int(t.arrays()["depth"].max()) if t.n_nodes else 0
        return t

    def close(self):
        if getattr(self, "h", None):
            lib().gs_taxtree_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    @staticmethod
    def _text(text):
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = np.frombuffer(bytes(text), dtype=np.uint8)
        return text, int(text.shape[0])

    def submit_nodes(self, text, last=False):
        """a chunk of whole nodes lines (bytes, a uint8 array, or a uint8 tensor on the handle's device) -> its report"""
        text, n = self._text(text)
        _ready(text)
        p, mem = _ptr(text) if n else (None, MEM_HOST)
        r = (C.c_int64 * 8)()
        _check(lib().gs_taxtree_submit_nodes(self.h, p, n, mem, int(bool(last)), r))
        return {"lines": r[0], "taken": r[2], "refused": r[3], "first_bad_line": r[4], "longest_line": r[5]}

    def append_nodes(self, text, last=False):
        """the same lines judged one by one on the host, at their place in the input order -> its report"""
        text, n = self._text(text)
        r = (C.c_int64 * 8)()
        _check(lib().gs_taxtree_append_nodes(self.h, _ptr(text)[0] if n else None, n, int(bool(last)), r))
        return {"lines": r[0], "taken": r[2], "refused": 0, "first_bad_line": -1, "longest_line": 0}

    def finish(self):
        """the tree -> {"nodes", "reached", "max_depth", "duplicates", "on_host", "cycle_nodes", "slots"}"""
        info = (C.c_int64 * 8)()
        _check(lib().gs_taxtree_finish_nodes(self.h, info))
        self.n_nodes, self.n_reached, self.max_depth, self.n_duplicates, self.on_host, self.n_cycle_nodes = tuple(info)[:6]
        return {"nodes": info[0], "reached": info[1], "max_depth": info[2], "duplicates": info[3], "on_host": info[4], "cycle_nodes": info[5],
                "slots": info[6]}

    def submit_names(self, text, last=False):
        """a chunk of whole names lines (bytes, a uint8 array, or a uint8 tensor on the handle's device), behind finish(), scanned
        on the device -> its report; a refused chunk wrote nothing and goes to append_names()"""
        text, n = self._text(text)
        _ready(text)
        p, mem = _ptr(text) if n else (None, MEM_HOST)
        r = (C.c_int64 * 8)()
        _check(lib().gs_taxtree_submit_names(self.h, p, n, mem, int(bool(last)), r))
        return {"lines": r[0], "taken": r[2], "refused": r[3], "first_bad_line": r[4], "longest_line": r[5]}

    def append_names(self, text, last=False):
        """the same lines judged one by one on the host, at their place in the input order (the only way on a tree that lives on
        the host)"""
        text, n = self._text(text)
        _check(lib().gs_taxtree_append_names(self.h, _ptr(text)[0] if n else None, n, int(bool(last))))

    def finish_times(self):
        """milliseconds of the last finish between events, if kernel_time(True) came before it -> (distinct ids and parents,
        child order, tree steps)"""
        ms = (C.c_double * 3)()
        _check(lib().gs_taxtree_finish_times(self.h, ms))
        return tuple(ms)

    def arrays(self):
        """-> {"taxids", "parent", "depth", "position", "subtree", "rank"}: int32[n_nodes] each"""
        out = {k: np.zeros(max(self.n_nodes, 1), dtype=np.int32) for k in ("taxids", "parent", "depth", "position", "subtree", "rank")}
        _check(lib().gs_taxtree_fetch(self.h, *(_ptr(out[k])[0] for k in ("taxids", "parent", "depth", "position", "subtree", "rank"))))
        return {k: v[:self.n_nodes] for k, v in out.items()}

    def names(self):
        """-> list of n_nodes names: bytes, or None for a node that no names line named"""
        off = np.zeros(self.n_nodes + 1, dtype=np.int64)
        _check(lib().gs_taxtree_fetch_names(self.h, _ptr(off)[0], None, 0))
        total = int(off[self.n_nodes])
        buf = np.zeros(max(total, 1), dtype=np.uint8)
        _check(lib().gs_taxtree_fetch_names(self.h, _ptr(off)[0], _ptr(buf)[0], total))
        raw = buf.tobytes()
        ends = [int(o) if o >= 0 else -1 - int(o) for o in off]
        return [raw[ends[i]:ends[i + 1]] if off[i] >= 0 else None for i in range(self.n_nodes)]

    def nodes_of(self, taxids, known=None):
        """tax ids -> their node indices; an id that names no node is dropped (TaxTree.getNodeByTaxId answers null)"""
        known = self.arrays()["taxids"] if known is None else known
        t = np.asarray(taxids, dtype=np.int64).reshape(-1)
        i = np.searchsorted(known, t)
        ok = (i < len(known)) & (known[np.minimum(i, len(known) - 1)] == t) if len(known) else np.zeros(len(t), dtype=bool)
        return i[ok].astype(np.int32)

    def select(self, requested, excluded=(), cut_rank=None):
        """the taxnodes set: requested / excluded node indices, cut_rank a rank name, an ordinal or None -> uint8[n_nodes]"""
        req = np.ascontiguousarray(requested, dtype=np.int32).reshape(-1)
        exc = np.ascontiguousarray(excluded, dtype=np.int32).reshape(-1)
        cut = -1 if cut_rank is None else RANK_NAMES.index(cut_rank) if isinstance(cut_rank, str) else int(cut_rank)
        out = np.zeros(max(self.n_nodes, 1), dtype=np.uint8)
        count = C.c_int64()
        _check(lib().gs_taxtree_select(self.h, _ptr(req)[0] if len(req) else None, len(req), _ptr(exc)[0] if len(exc) else None, len(exc), cut,
                                       _ptr(out)[0], C.byref(count)))
        self.n_selected = count.value
        return out[:self.n_nodes]

    def small_tree(self, flagged):
        """flagged: uint8[n_nodes] (host array or device tensor) or int32[n_nodes] with > 0 meaning flagged (the regions of an
        accession map) -> {"node_of_vi", "parent_vi", "depth", "position"}: int32[n_small] each, the root first"""
        if not hasattr(flagged, "device") or isinstance(flagged, np.ndarray):
            flagged = np.ascontiguousarray(flagged)
            if flagged.dtype not in (np.uint8, np.int32):
                flagged = flagged.astype(np.uint8)
        if int(flagged.shape[0]) != self.n_nodes:
            raise ValueError("one flag per node")
        _ready(flagged)
        p, mem = _ptr(flagged)
        size = int(flagged.element_size()) if hasattr(flagged, "element_size") else flagged.dtype.itemsize
        cap = max(self.n_reached, 1)
        out = {k: np.zeros(cap, dtype=np.int32) for k in ("node_of_vi", "parent_vi", "depth", "position")}
        n_small = C.c_int32()
        _check(lib().gs_taxtree_small(self.h, p, size, mem, C.byref(n_small), *(_ptr(out[k])[0] for k in ("node_of_vi", "parent_vi", "depth", "position"))))
        return {k: v[:n_small.value] for k, v in out.items()}

    def regions_below(self, regions, selected, limit, check_rank=None, refseq_db=True, rna_only=False):
        """the taxfromgenbank set.  regions: int32[n_nodes], entries of an accession map per node itself (DeviceAccessionMap.fetch's
        regions; a host array or a tensor on the tree's device); selected: the taxnodes set as node indices, or as select()'s
        uint8[n_nodes]; limit: refSeq.limitForGenbankAccess; check_rank: refSeq.limitForGenbankRank as a rank name, an ordinal or
        None for any rank -> (below, inclusive): the selected nodes of that rank whose count is below limit, ascending, and
        int32[n_nodes], the count per node with everything below it.  What the goal puts in front is applied here: refseq_db False
        (refseq.filldb off) gives the whole selection, rna_only (SeqType.RNA) or limit <= 0 an empty set"""
        sel = np.asarray(selected)
        if sel.dtype == np.uint8 and sel.shape == (self.n_nodes,):
            sel = np.flatnonzero(sel)
        sel = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1)
        if not hasattr(regions, "device") or isinstance(regions, np.ndarray):
            regions = np.ascontiguousarray(regions, dtype=np.int32)
        if int(regions.shape[0]) != self.n_nodes:
            raise ValueError("one region count per node")
        _ready(regions)
        p, mem = _ptr(regions)
        rank = -1 if check_rank is None else RANK_NAMES.index(check_rank) if isinstance(check_rank, str) else int(check_rank)
        incl = np.zeros(max(self.n_nodes, 1), dtype=np.int32)
        below = np.zeros(max(len(sel), 1), dtype=np.int32)
        n_below = C.c_int64()
        _check(lib().gs_taxtree_regions_below(self.h, p, mem, _ptr(sel)[0] if len(sel) else None, len(sel), int(limit), rank, _ptr(incl)[0],
                                              _ptr(below)[0], C.byref(n_below)))
        incl = incl[:self.n_nodes]
        if not refseq_db:
            return np.unique(sel), incl
        if rna_only or limit <= 0:
            return below[:0], incl
        return below[:n_below.value], incl

    def kernel_time(self, profile=True):
        """(launches, milliseconds) of the scan, finish, select, small and regions kernels so far; switches their timing on or off"""
        n, ms = C.c_int64(), C.c_double()
        _check(lib().gs_taxtree_kernel_time(self.h, int(profile), C.byref(n), C.byref(ms)))
        return n.value, ms.value
