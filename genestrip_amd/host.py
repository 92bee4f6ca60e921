"""ctypes binding of include/gshost.h (libgshost.so): the C++ host layer above the C ABI -- FASTQ/FASTA ingest with
the reference's record semantics, the runMatcher / runFilter file pipelines and the CSV report."""
import ctypes as C
import os
import threading

import numpy as np

from . import binding as _b

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class _ReadBatch(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("seq", C.c_void_p), ("seq_off", C.c_void_p), ("desc", C.c_void_p),
                ("desc_off", C.c_void_p), ("qual", C.c_void_p), ("qual_off", C.c_void_p), ("first_read_no", C.c_int64)]


class _MatchOpts(C.Structure):
    _fields_ = [("filtered_path", C.c_char_p), ("kraken_out_path", C.c_char_p), ("write_all", C.c_int32),
                ("taxids", C.POINTER(C.c_char_p)), ("batch_reads", C.c_int64), ("with_probs", C.c_int32),
                ("max_contig_desc", C.c_void_p), ("max_contig_desc_stride", C.c_int32)]


class Totals(C.Structure):
    _fields_ = [("reads", C.c_int64), ("kmers", C.c_int64), ("bps", C.c_int64), ("filtered_reads", C.c_int64),
                ("seconds_total", C.c_double), ("seconds_parse", C.c_double), ("seconds_gpu", C.c_double)]


class _TaxInfo(C.Structure):
    _fields_ = [("n_values", C.c_int32), ("parent_vi", C.c_void_p), ("position", C.c_void_p),
                ("taxids", C.POINTER(C.c_char_p)), ("names", C.POINTER(C.c_char_p)), ("ranks", C.POINTER(C.c_char_p)),
                ("db_kmers", C.c_void_p), ("db_kmers_total", C.c_int64), ("max_contig_desc", C.POINTER(C.c_char_p)),
                ("max_kmer_counts", C.c_void_p), ("max_kmer_res_counts", C.c_int32)]


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    _b.lib()  # loads libgsgpu.so (and the HIP runtime) first
    path = os.path.join(_HERE, "libgshost.so")
    if not os.path.exists(path):
        raise _b.GsError(-6, f"{path} is missing: build it with `make -C genestrip_amd/csrc`")
    L = C.CDLL(path)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    sig = {
        "gs_fastq_open": (ci, [vp, C.c_char_p, ci, ci]), "gs_fastq_next": (ci, [vp, i64, i64, vp]),
        "gs_fastq_totals": (ci, [vp, vp, vp, vp]), "gs_fastq_close": (ci, [vp]),
        "gs_host_match_files": (ci, [vp, vp, vp, ci, vp, vp, vp, vp]),
        "gs_host_match_into": (ci, [vp, vp, vp, ci, vp, vp, vp]),
        "gs_host_match_run": (ci, [vp, vp, vp, ci, vp, vp]),
        "gs_host_match_files_multi": (ci, [vp, ci, vp, vp, ci, vp, vp, vp]),
        "gs_host_stat": (C.c_int64, [ci]),
        "gs_host_release_pools": (ci, []),
        "gs_host_filter_files": (ci, [vp, ci, ci, C.c_double, vp, ci, C.c_char_p, C.c_char_p, ci, vp]),
        "gs_host_extract_files": (ci, [ci, C.c_char_p, ci, vp, ci, C.c_char_p, vp]),
        "gs_host_fasta2fastq": (ci, [ci, vp, ci, C.c_char_p, vp]),
        "gs_host_write_csv": (ci, [C.c_char_p, vp, vp, vp, vp]),
        "gs_host_write_quality_csv": (ci, [C.c_char_p, vp, vp, vp]),
        "gs_host_kraken_count_files": (ci, [ci, vp, ci, vp, ci, C.c_char_p, vp, C.c_int32, vp, i64, vp, vp]),
        "gs_host_genome_files": (ci, [vp, ci, ci, vp, vp, vp, vp, vp]),
        "gs_host_accmap_files": (ci, [vp, ci, ci, vp, ci, vp, vp]),
        "gs_host_asmsum_files": (ci, [vp, ci, ci, vp, C.c_int32, vp, vp]),
        "gs_host_genome_files_mapped": (ci, [vp, ci, ci, vp, ci, vp, vp, vp, vp, vp]),
        "gs_host_genome_files_into": (ci, [vp, ci, ci, vp, ci, vp, vp, C.c_int32, ci, vp, ci, vp]),
        "gs_host_taxtree_files": (ci, [ci, C.c_char_p, C.c_char_p, vp, vp]),
        "gs_host_read_taxids_file": (ci, [C.c_char_p, vp, vp, vp, vp, i64]),
        "gs_host_write_kraken_csv": (ci, [C.c_char_p, vp, C.c_int32, vp, i64]),
        "gs_host_db2fastq": (ci, [vp, vp, C.c_char_p, C.c_int32, ci, C.c_char_p, vp]),
        "gs_host_last_error": (C.c_char_p, []), "gs_host_java_double": (ci, [C.c_double, vp, ci]),
        "gs_host_gunzip": (ci, [vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]),
        "gs_host_gunzip_parallel": (ci, [vp, C.c_size_t, vp, C.c_size_t, vp, ci, C.c_size_t, C.c_size_t]),
        "gs_host_control_create": (ci, [vp, vp, vp, C.c_int32]), "gs_host_control_destroy": (ci, [vp]),
        "gs_host_control_cancel": (ci, [vp]), "gs_host_control_snapshot": (ci, [vp, vp, vp]),
        "gs_host_control_attach": (ci, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    _LIB = L
    return L


def _check(rc, **partial):
    """raises for a non-zero status; GS_E_CANCELLED (-8) as Cancelled, carrying `partial` -- what the wrapper would have returned"""
    if rc == CANCELLED:
        raise Cancelled(**partial)
    if rc != 0:
        msg = (lib().gs_host_last_error() or b"").decode(errors="replace")
        if not msg:
            msg = (_b.lib().gs_last_error() or b"").decode(errors="replace")
        raise _b.GsError(rc, msg)


CANCELLED = -8  # GS_E_CANCELLED


class Cancelled(_b.GsError):
    """a file-level call was stopped on request (Control): the partial results the wrapper would have returned -- table, dtable,
    totals, ... -- are attributes; they cover exactly the reads of the last progress records"""

    def __init__(self, **partial):
        super().__init__(CANCELLED, "cancelled")
        self.partial = partial
        for name, value in partial.items():
            setattr(self, name, value)


class Progress(C.Structure):
    """gs_host_progress"""
    _fields_ = [("file", C.c_int32), ("n_files", C.c_int32), ("file_done", C.c_int32), ("files_done", C.c_int32),
                ("file_bytes_done", C.c_int64), ("file_bytes_total", C.c_int64), ("file_reads", C.c_int64),
                ("total_bytes_done", C.c_int64), ("total_bytes_total", C.c_int64), ("total_reads", C.c_int64),
                ("seconds_file", C.c_double), ("seconds_total", C.c_double)]

    def copy(self):
        r = Progress()
        C.memmove(C.byref(r), C.byref(self), C.sizeof(Progress))
        return r

    def __repr__(self):
        return "Progress(" + ", ".join(f"{f}={getattr(self, f)}" for f, _ in self._fields_) + ")"


_PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(Progress))
_THREAD = threading.local()


def _attached():
    """the Controls this thread has entered, innermost last"""
    if not hasattr(_THREAD, "stack"):
        _THREAD.stack = []
    return _THREAD.stack


class Control:
    """Progress and cancellation of the file-level calls (match_files, match_run, match_files_into, filter_files, extract_files,
    fasta2fastq, kraken_count_files, genome_files, genome_files_mapped, genome_files_into, accmap_files, assembly_summary_files,
    taxtree_files) that THIS thread makes inside the `with` block:

        with host.Control(callback=lambda p: p.total_reads > 10**9, every_ms=200) as ctl:
            table, dtable, tot = host.match_files(store, paths)

    callback(record) runs on the calling thread with a Progress (a copy: keep it if you like); a true return value stops the call,
    .cancel() does the same from any thread, .snapshot() -> (Progress, cancelled) reads the latest record from any thread.  A
    stopped call raises Cancelled, which carries the partial results.  An exception raised by the callback stops the call and is
    raised again when the block is left."""

    def __init__(self, callback=None, every_ms=0):
        self.callback, self.every_ms = callback, int(every_ms)
        self.h = None
        self._raised = None
        self._fn = _PROGRESS_FN(self._call) if callback is not None else None

    def _call(self, _user, p):
        try:
            return 1 if self.callback(p.contents.copy()) else 0
        except BaseException as e:  # noqa: BLE001 -- nothing may leave through the C frames
            self._raised = e
            return 1

    def __enter__(self):
        h = C.c_void_p()
        _check(lib().gs_host_control_create(C.byref(h), C.cast(self._fn, C.c_void_p) if self._fn else None, None, self.every_ms))
        rc = lib().gs_host_control_attach(h)
        if rc != 0:
            lib().gs_host_control_destroy(h)
            _check(rc)
        self.h = h
        stack = _attached()
        stack.append(self)
        return self

    def __exit__(self, etype, exc, tb):
        stack = _attached()
        if self in stack:
            stack.remove(self)
        outer = stack[-1].h if stack else None  # (a Control inside another: the outer one is this thread's again)
        lib().gs_host_control_attach(outer)
        h, self.h = self.h, None
        _check(lib().gs_host_control_destroy(h))
        if self._raised is not None and (etype is None or issubclass(etype, Cancelled)):
            raised, self._raised = self._raised, None
            raise raised
        return False

    def cancel(self):
        _check(lib().gs_host_control_cancel(self.h))

    def snapshot(self):
        p, flag = Progress(), C.c_int32(0)
        _check(lib().gs_host_control_snapshot(self.h, C.byref(p), C.byref(flag)))
        return p, bool(flag.value)


def _cstr_array(items):
    if items is None:
        return None
    arr = (C.c_char_p * len(items))()
    for i, s in enumerate(items):
        arr[i] = None if s is None else (s if isinstance(s, bytes) else str(s).encode())
    return arr


class FastqReader:
    """AbstractFastqReader's record semantics (FASTQ or FASTA, gzip by content) as batches of numpy arrays"""

    def __init__(self, path, k=31, fasta=None):
        self.h = C.c_void_p()
        _check(lib().gs_fastq_open(C.byref(self.h), str(path).encode(), -1 if fasta is None else int(fasta), k))

    def next_batch(self, max_reads=1 << 20, max_bytes=1 << 30):
        b = _ReadBatch()
        _check(lib().gs_fastq_next(self.h, max_reads, max_bytes, C.byref(b)))
        n = b.n_reads
        if n == 0:
            return None

        def arr(ptr, ctype, cnt):
            if cnt == 0:
                return np.zeros(0, dtype=np.dtype(ctype))
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(cnt,)).copy()
        so, do, qo = (arr(p, C.c_uint64, n + 1) for p in (b.seq_off, b.desc_off, b.qual_off))
        return dict(n_reads=n, first_read_no=b.first_read_no, seq_off=so, desc_off=do, qual_off=qo,
                    seq=arr(b.seq, C.c_uint8, int(so[-1])), desc=arr(b.desc, C.c_uint8, int(do[-1])),
                    qual=arr(b.qual, C.c_uint8, int(qo[-1])))

    def totals(self):
        r, k, p = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(lib().gs_fastq_totals(self.h, C.byref(r), C.byref(k), C.byref(p)))
        return r.value, k.value, p.value

    def close(self):
        if getattr(self, "h", None):
            lib().gs_fastq_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def release_pools():
    """gs_host_release_pools: the page-locked blocks and device decoders the host layer keeps from call to call are freed"""
    _check(lib().gs_host_release_pools())


def match_files(store, paths, config=None, filtered_path=None, kraken_out_path=None, write_all=True, taxids=None,
                batch_reads=0, with_probs=False, max_contig_desc=False):
    """FastqKMerMatcher.runMatcher over files: returns (table, dtable, Totals); with_probs = the reference's withProbs
    (written reads keep their quality lines); max_contig_desc=True: a fourth result, the names of the reads that hold the longest
    contigs (list of bytes per value index)"""
    cfg = (config or _b.MatchConfig())._c()
    parr = _cstr_array(list(paths))
    tarr = _cstr_array(taxids)
    nv = store.n_values
    stride = 128
    descs = np.zeros((nv, stride), dtype=np.uint8) if max_contig_desc else None
    opts = _MatchOpts(None if filtered_path is None else str(filtered_path).encode(),
                      None if kraken_out_path is None else str(kraken_out_path).encode(), int(write_all),
                      tarr, batch_reads, int(with_probs), None if descs is None else descs.ctypes.data_as(C.c_void_p), stride)
    table = np.zeros((nv, _b.N_COLS), dtype=np.int64)
    dtable = np.zeros((nv, _b.N_DCOLS), dtype=np.float64)
    tot = Totals()
    _check(lib().gs_host_match_files(store.h, C.byref(cfg), parr, len(paths), C.byref(opts),
                                     table.ctypes.data_as(C.c_void_p), dtable.ctypes.data_as(C.c_void_p), C.byref(tot)),
           table=table, dtable=dtable, totals=tot)
    if descs is not None:
        return table, dtable, tot, [bytes(row).split(b"\0", 1)[0] for row in descs]
    return table, dtable, tot


def match_run(matcher, paths, filtered_path=None, kraken_out_path=None, write_all=True, taxids=None, batch_reads=0,
              with_probs=False):
    """gs_host_match_run: the files into `matcher`'s own run (no finish: matcher.finish() gives the table, matcher.reset() clears
    it), per-read outputs included, one file after the other with running read numbers; -> Totals"""
    parr = _cstr_array(list(paths))
    tarr = _cstr_array(taxids)
    opts = _MatchOpts(None if filtered_path is None else str(filtered_path).encode(),
                      None if kraken_out_path is None else str(kraken_out_path).encode(), int(write_all),
                      tarr, batch_reads, int(with_probs), None, 0)
    tot = Totals()
    _check(lib().gs_host_match_run(matcher.h, matcher.store.h, parr, len(paths), C.byref(opts), C.byref(tot)), totals=tot)
    return tot


def stat(which=0):
    """gs_host_stat: 0 = chunks that went through the general (multi-line) FASTQ device path in this process so far; 1 = FASTA / general
    FASTQ chunks the filter goal handled on the device; 2 = four-line chunks whose Kraken-style lines were written on the device; 3 = FASTA /
    general FASTQ chunks of any goal whose per-read output was written on the device (GS_DEVICE_RECORDS=0 keeps them on the host); 5 = chunks
    of Kraken-style lines that kraken_count_files counted on the device"""
    return int(lib().gs_host_stat(which))


def match_files_multi(stores, paths, config=None):
    """gs_host_match_files_multi: the files of a sample over several store replicas (one per device) of this process"""
    cfg = (config or _b.MatchConfig())._c()
    parr = _cstr_array(list(paths))
    darr = (C.c_void_p * len(stores))(*[s.h for s in stores])
    nv = stores[0].n_values
    table = np.zeros((nv, _b.N_COLS), dtype=np.int64)
    dtable = np.zeros((nv, _b.N_DCOLS), dtype=np.float64)
    tot = Totals()
    _check(lib().gs_host_match_files_multi(darr, len(stores), C.byref(cfg), parr, len(paths),
                                           table.ctypes.data_as(C.c_void_p), dtable.ctypes.data_as(C.c_void_p), C.byref(tot)))
    return table, dtable, tot


def match_files_into(matcher, paths, file_index):
    """the given files into `matcher`'s run (no finish): returns (reads per file, Totals); file_index = position of each
    file in the global file order (read numbers are file_index << 32 | read in file)"""
    parr = _cstr_array(list(paths))
    fi = np.ascontiguousarray(file_index, dtype=np.int32)
    counts = np.zeros(max(len(fi), 1), dtype=np.int64)
    tot = Totals()
    _check(lib().gs_host_match_into(matcher.h, matcher.store.h, parr, len(fi), fi.ctypes.data_as(C.c_void_p),
                                    counts.ctypes.data_as(C.c_void_p), C.byref(tot)), reads_of_file=counts[:len(fi)], totals=tot)
    return counts[:len(fi)], tot


def filter_files(bloom, k, paths, min_pos_count=1, positive_ratio=0.2, filtered_path=None, rest_path=None,
                 with_probs=False):
    parr = _cstr_array(list(paths))
    tot = Totals()
    _check(lib().gs_host_filter_files(bloom.h, k, min_pos_count, positive_ratio, parr, len(paths),
                                      None if filtered_path is None else str(filtered_path).encode(),
                                      None if rest_path is None else str(rest_path).encode(), int(with_probs),
                                      C.byref(tot)), totals=tot)
    return tot


def extract_files(key, paths, out_path, k=31, device=0):
    """the extract goal: every read of the files whose descriptor starts with `key` -> out_path (.gz: BGZF), written as
    ReadEntry.write with qualities; -> Totals (filtered_reads = reads written)"""
    parr = _cstr_array(list(paths))
    tot = Totals()
    _check(lib().gs_host_extract_files(int(device), key if isinstance(key, bytes) else str(key).encode(), int(k), parr, len(paths),
                                       str(out_path).encode(), C.byref(tot)), totals=tot)
    return tot


def fasta2fastq(paths, out_path, device=0):
    """the fasta2fastq goal: the FASTA files, in order, as one four-line FASTQ file with '~' qualities (.gz: BGZF); -> records"""
    parr = _cstr_array(list(paths))
    n = C.c_int64(0)
    rc = lib().gs_host_fasta2fastq(int(device), parr, len(paths), str(out_path).encode(), C.byref(n))
    _check(rc, records=n.value)
    return n.value


def write_csv(path, parent_vi, taxids, db_kmers, db_kmers_total, table, dtable, totals, names=None, ranks=None,
              position=None, max_contig_desc=None, max_kmer_counts=None):
    """MatchingResult.completeResults + ResultReporter.printMatchResult"""
    pv = np.ascontiguousarray(parent_vi, dtype=np.int32)
    dk = np.ascontiguousarray(db_kmers, dtype=np.int64)
    pos = None if position is None else np.ascontiguousarray(position, dtype=np.int32)
    keep = [_cstr_array(taxids), _cstr_array(names), _cstr_array(ranks), _cstr_array(max_contig_desc)]
    mc = None if max_kmer_counts is None else np.ascontiguousarray(max_kmer_counts, dtype=np.int16)
    info = _TaxInfo(len(pv), pv.ctypes.data_as(C.c_void_p), None if pos is None else pos.ctypes.data_as(C.c_void_p),
                    keep[0], keep[1], keep[2], dk.ctypes.data_as(C.c_void_p), db_kmers_total, keep[3],
                    None if mc is None else mc.ctypes.data_as(C.c_void_p), 0 if mc is None else mc.shape[1])
    t = np.ascontiguousarray(table, dtype=np.int64)
    d = np.ascontiguousarray(dtable, dtype=np.float64)
    _check(lib().gs_host_write_csv(str(path).encode(), C.byref(info), t.ctypes.data_as(C.c_void_p),
                                   d.ctypes.data_as(C.c_void_p), C.byref(totals)))


def write_quality_csv(path, parent_vi, taxids, counts, present, names=None, ranks=None, position=None):
    """the dbquality goal's CSV (DBQualityCountsGoal's rank aggregation + DBQualityCSVGoal.makeFile) from
    DeviceDbQuality.finish(): counts int64[n_values, 3] = tp, tp+fp, tp+fn and present uint8[n_values]"""
    pv = np.ascontiguousarray(parent_vi, dtype=np.int32)
    c = np.ascontiguousarray(counts, dtype=np.int64)
    pr = np.ascontiguousarray(present, dtype=np.uint8)
    if c.shape != (len(pv), 3) or pr.shape != (len(pv),) or len(taxids) != len(pv):
        raise ValueError("counts must be [n_values, 3], present and taxids [n_values]")
    pos = None if position is None else np.ascontiguousarray(position, dtype=np.int32)
    keep = [_cstr_array(taxids), _cstr_array(names), _cstr_array(ranks)]
    info = _TaxInfo(len(pv), pv.ctypes.data_as(C.c_void_p), None if pos is None else pos.ctypes.data_as(C.c_void_p),
                    keep[0], keep[1], keep[2], None, 0, None, None, 0)
    _check(lib().gs_host_write_quality_csv(str(path).encode(), C.byref(info), c.ctypes.data_as(C.c_void_p),
                                           pr.ctypes.data_as(C.c_void_p)))


def db2fastq(store, taxids, project, path, select=None, with_desc=True):
    """the db2fastq goal (KMerFastqGenerator.generateFastq): the stored k-mers of value `select` (with_desc: and its subtree;
    None: all, the goal's "total" file) as FASTQ, gzip (BGZF) when the name ends in .gz / .gzip.  taxids: the tax id string of
    every value index.  Returns the number of records written."""
    if len(taxids) != store.n_values:
        raise ValueError("taxids must have one entry per value index")
    tarr = _cstr_array(list(taxids))
    n = C.c_int64(0)
    _check(lib().gs_host_db2fastq(store.h, tarr, str(project).encode(), -1 if select is None else int(select), int(bool(with_desc)),
                                  str(path).encode(), C.byref(n)))
    return n.value


def gunzip(data, expected_size, block=1 << 20):
    """the ingest path's gzip decoder on bytes (test hook): returns the decoded bytes"""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty(max(int(expected_size), 1), dtype=np.uint8)
    n = C.c_size_t(0)
    _check(lib().gs_host_gunzip(src.ctypes.data_as(C.c_void_p) if len(src) else None, len(src), out.ctypes.data_as(C.c_void_p),
                                int(expected_size), C.byref(n), int(block)))
    return out[:n.value].tobytes()


def gunzip_parallel(data, expected_size, threads=4, chunk=1 << 20, block=1 << 20):
    """the multi-threaded gzip decoder of the text path on bytes (test hook)"""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty(max(int(expected_size), 1), dtype=np.uint8)
    n = C.c_size_t(0)
    _check(lib().gs_host_gunzip_parallel(src.ctypes.data_as(C.c_void_p) if len(src) else None, len(src),
                                         out.ctypes.data_as(C.c_void_p), int(expected_size), C.byref(n), int(threads), int(chunk), int(block)))
    return out[:n.value].tobytes()


def java_double(v):
    buf = C.create_string_buffer(64)
    _check(lib().gs_host_java_double(float(v), buf, 64))
    return buf.value.decode()


class KrakenTotals(C.Structure):
    _fields_ = [("lines", C.c_int64), ("counted_tokens", C.c_int64), ("a_tokens", C.c_int64), ("long_lines", C.c_int64),
                ("device_chunks", C.c_int64), ("host_chunks", C.c_int64), ("seconds_total", C.c_double)]


_KRAKEN_KEY_STRIDE = 24


def kraken_count_files(paths, only=None, csv=None, device=0):
    """The krakencount goal over Kraken-style output files (plain or gzip; ours, Kraken's, KrakenUniq's), all into one table:
    (rows, totals) with rows = [(tax id bytes, reads, kmers, kmers in matching reads)] in the reference's order.  only: keep the rows
    of these tax ids; csv: also write the krakenres CSV there (.gz: gzip).  Chunks of whole lines are counted on the device, what it
    refuses by a line-by-line restatement of the reference; GS_HOST_FAST=0 sends everything through the latter."""
    parr = _cstr_array([os.fspath(p) for p in paths])
    oarr = _cstr_array(list(only)) if only is not None else None
    tot = KrakenTotals()
    n = C.c_int64(0)
    cap, stride = 1 << 12, _KRAKEN_KEY_STRIDE
    csv_b = None if csv is None else os.fspath(csv).encode()
    while True:
        keys = np.zeros((cap, stride), dtype=np.uint8)
        cnt = np.zeros((cap, 3), dtype=np.int64)
        rc = lib().gs_host_kraken_count_files(int(device), parr, len(paths), oarr, 0 if only is None else len(oarr), csv_b,
                                              keys.ctypes.data_as(C.c_void_p), stride, cnt.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(tot))
        if rc != 0 and n.value > 0 and (n.value > cap or stride < 4096) and b"no room" in (lib().gs_host_last_error() or b""):
            cap, stride = max(cap, n.value), (stride if n.value > cap else stride * 16)  # (more rows than guessed, or very long keys)
            continue
        if rc != CANCELLED:
            _check(rc)
        break
    rows = [(bytes(keys[i]).split(b"\0", 1)[0], int(cnt[i, 0]), int(cnt[i, 1]), int(cnt[i, 2])) for i in range(n.value)]
    totals = {f: getattr(tot, f) for f, _ in KrakenTotals._fields_}
    _check(rc, rows=rows, totals=totals)
    return rows, totals


def write_kraken_csv(path, rows):
    """taxid;reads;kmers;kmers in matching reads -- the krakenres file of rows as kraken_count_files returns them"""
    stride = max([len(r[0]) for r in rows] + [0]) + 1
    keys = np.zeros((max(len(rows), 1), stride), dtype=np.uint8)
    cnt = np.zeros((max(len(rows), 1), 3), dtype=np.int64)
    for i, (k, *v) in enumerate(rows):
        keys[i, :len(k)] = np.frombuffer(bytes(k), dtype=np.uint8)
        cnt[i] = v
    _check(lib().gs_host_write_kraken_csv(os.fspath(path).encode(), keys.ctypes.data_as(C.c_void_p), stride, cnt.ctypes.data_as(C.c_void_p), len(rows)))


class GenomeTotals(C.Structure):
    _fields_ = [("records", C.c_int64), ("kept_records", C.c_int64), ("text_bytes", C.c_int64), ("kept_bases", C.c_int64),
                ("chunks", C.c_int64), ("host_chunks", C.c_int64), ("max_line_bytes", C.c_int64), ("seconds_total", C.c_double)]


_RESOLVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_RESOLVE_NODES_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p)
_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)
_CALLBACK_RAISED = -1000


def genome_files(paths, resolve, sink, device=0, _mapped=None):
    """gs_host_genome_files: genome FASTA files (plain, gzip, BGZF) -> the regions of a build.  resolve(file, first_record, headers)
    gets the header lines (a list of bytes, '>' included) of a batch of records and returns one value index per record (< 0: skip),
    or a non-zero int as its error code; sink(seq, offsets, vi) gets the kept regions -- seq / offsets as device views or numpy
    arrays, in both cases what DeviceDbBuilder.add, DeviceDbSizer.add, DeviceDbUpdater.add and DeviceDbQuality.add take, valid
    until it returns -- and may return a non-zero int as well.  Such a code ends the walk and comes back as GsError(code); use
    POSITIVE codes: -1 .. -8 are the library's own GS_E_* codes and are reported with the library's last message.  An exception
    raised inside a callback ends the walk and is raised again.  -> GenomeTotals"""
    raised = []

    def _resolve(_user, file, first, n, hdr, hoff, vi):
        try:
            off = np.ctypeslib.as_array(C.cast(hoff, C.POINTER(C.c_uint64)), (n + 1,))
            raw = C.string_at(hdr, int(off[n]))
            got = resolve(file, first, [raw[int(off[i]):int(off[i + 1])] for i in range(n)])
            if isinstance(got, (int, np.integer)) and not isinstance(got, bool):
                return int(got)
            got = np.ascontiguousarray(got, dtype=np.int32)
            if len(got) != n:
                raise ValueError("resolve must return one value index per record")
            C.memmove(vi, got.ctypes.data, 4 * n)
            return 0
        except BaseException as e:  # noqa: BLE001 -- nothing may leave through the C frames
            raised.append(e)
            return _CALLBACK_RAISED

    def _sink(_user, seq, off, vi, n, mem):
        try:
            v = np.ctypeslib.as_array(C.cast(vi, C.POINTER(C.c_int32)), (n,)).copy()
            if mem == _b.MEM_DEVICE:
                o = _b.DeviceView(off, n + 1, np.uint64, device)
                total = int(o.numpy()[-1])
                s = _b.DeviceView(seq, total, np.uint8, device)
            else:
                o = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (n + 1,))
                s = np.ctypeslib.as_array(C.cast(seq, C.POINTER(C.c_uint8)), (max(int(o[n]), 1),))[:int(o[n])]
            got = sink(s, o, v)
            return int(got) if isinstance(got, (int, np.integer)) and not isinstance(got, bool) else 0
        except BaseException as e:  # noqa: BLE001
            raised.append(e)
            return _CALLBACK_RAISED

    def _resolve_nodes(_user, file, first, n, node, vi):
        try:
            got = resolve(file, first, np.ctypeslib.as_array(C.cast(node, C.POINTER(C.c_int32)), (n,)).copy())
            if isinstance(got, (int, np.integer)) and not isinstance(got, bool):
                return int(got)
            got = np.ascontiguousarray(got, dtype=np.int32)
            if len(got) != n:
                raise ValueError("resolve must return one value index per record")
            C.memmove(vi, got.ctypes.data, 4 * n)
            return 0
        except BaseException as e:  # noqa: BLE001
            raised.append(e)
            return _CALLBACK_RAISED

    paths = [os.fspath(p) for p in paths]
    arr, n = _cstr_array(paths), len(paths)
    t = GenomeTotals()
    s_fn = _SINK_FN(_sink)
    if _mapped is None:
        r_fn = _RESOLVE_FN(_resolve)
        rc = lib().gs_host_genome_files(arr, n, device, r_fn, None, s_fn, None, C.byref(t))
    else:
        r_fn = _RESOLVE_NODES_FN(_resolve_nodes)
        rc = lib().gs_host_genome_files_mapped(arr, n, device, _mapped[0].h, int(bool(_mapped[1])), r_fn, None, s_fn, None, C.byref(t))
    if raised:
        raise raised[0]
    if rc > 0 or rc < CANCELLED:
        raise _b.GsError(rc, "a callback of genome_files ended the walk with this code")
    _check(rc, totals=t)
    return t


def genome_files_mapped(paths, accession_map, resolve, sink, complete_only=False, device=0):
    """gs_host_genome_files_mapped: genome_files with an accession map (genestrip_amd.DeviceAccessionMap, finished) in front of the
    resolver.  The header lines of a chunk are looked up on the device, where the scan left them; resolve(file, first_record, nodes)
    gets one node per record (int32 array, -1: none) instead of header text and returns one value index per record as in
    genome_files.  -> GenomeTotals"""
    return genome_files(paths, resolve, sink, device=device, _mapped=(accession_map, complete_only))


INTO_SIZE, INTO_BUILD, INTO_UPDATE, INTO_QUALITY = 0, 1, 2, 3  # GS_HOST_INTO_*
_INTO_KINDS = {"DeviceDbSizer": INTO_SIZE, "DeviceDbBuilder": INTO_BUILD, "DeviceDbUpdater": INTO_UPDATE, "DeviceDbQuality": INTO_QUALITY}


def genome_files_into(paths, target, vi_of_node, accession_map=None, node_of_file=None, complete_only=False, update=False, kind=None,
                      device=0):
    """gs_host_genome_files_into: genome_files_mapped without callbacks.  vi_of_node: the value index per tree node (< 0: skip);
    node_of_file: None, or per file a node (>= 0: every record of the file counts for it, no lookup; < 0: look the record up in
    accession_map, a finished DeviceAccessionMap); target: a DeviceDbSizer, DeviceDbBuilder (update: its add's flag),
    DeviceDbUpdater or DeviceDbQuality, whose add receives the kept regions (kind: one of INTO_* for any other object with a
    handle `h`).  Limits per tax id and the finer-node options are not served.  -> GenomeTotals"""
    if kind is None:
        kind = _INTO_KINDS.get(type(target).__name__)
        if kind is None:
            raise TypeError("target must be a DeviceDbSizer, DeviceDbBuilder, DeviceDbUpdater or DeviceDbQuality (or give kind)")
    paths = [os.fspath(p) for p in paths]
    vi = np.ascontiguousarray(vi_of_node, dtype=np.int32)
    nof = None if node_of_file is None else np.ascontiguousarray(node_of_file, dtype=np.int32)
    if nof is not None and len(nof) != len(paths):
        raise ValueError("one node_of_file entry per path")
    t = GenomeTotals()
    rc = lib().gs_host_genome_files_into(_cstr_array(paths), len(paths), int(device), accession_map.h if accession_map is not None else None,
                                         int(bool(complete_only)), nof.ctypes.data_as(C.c_void_p) if nof is not None and len(nof) else None,
                                         vi.ctypes.data_as(C.c_void_p) if len(vi) else None, len(vi), int(kind),
                                         getattr(target, "h", None), int(bool(update)), C.byref(t))
    _check(rc, totals=t)
    return t


class AccmapTotals(C.Structure):
    _fields_ = [("lines", C.c_int64), ("passing", C.c_int64), ("put", C.c_int64), ("device_chunks", C.c_int64), ("host_chunks", C.c_int64),
                ("seconds_total", C.c_double)]


def accmap_files(paths, known_taxids, categories, statuses, seq_type="GENOMIC", count_only=False, device=0, reserve_entries=0):
    """gs_host_accmap_files: the accmapsize / accmap goals over RefSeq catalog files (plain, gzip, BGZF), all into one map ->
    (DeviceAccessionMap or None if count_only, totals); totals["passing"] is the accmapsize number.  Chunks of whole lines are scanned
    on the device, what it refuses by a line-by-line restatement of the reference; GS_HOST_FAST=0 sends everything through the latter
    and gives a host-only map.  A stop on request raises Cancelled: no map."""
    cfg, known = _b.DeviceAccessionMap.config(known_taxids, categories, statuses, seq_type, reserve_entries)
    paths = [os.fspath(p) for p in paths]
    tot = AccmapTotals()
    h = C.c_void_p()
    rc = lib().gs_host_accmap_files(_cstr_array(paths), len(paths), int(device), C.byref(cfg), int(bool(count_only)), C.byref(h), C.byref(tot))
    totals = {f: getattr(tot, f) for f, _ in AccmapTotals._fields_}
    _check(rc, totals=totals)
    if count_only:
        return None, totals
    m = _b.DeviceAccessionMap._wrap(h, known)
    m.n_entries, m.n_passing = totals["put"], totals["passing"]
    return m, totals


class AsmsumTotals(C.Structure):
    _fields_ = [("lines", C.c_int64), ("counted", C.c_int64), ("kept", C.c_int64), ("picked", C.c_int64), ("nodes", C.c_int64),
                ("device_chunks", C.c_int64), ("host_chunks", C.c_int64), ("seconds_total", C.c_double)]


def assembly_summary_files(paths, known_taxids, selected=None, qualities=("COMPLETE_LATEST", "CHROMOSOME_LATEST"), reference_only=False,
                           use_species_taxid=False, max_per_taxid=1, device=0):
    """gs_host_asmsum_files: the fastasgenbank goal over Genbank assembly summary files (plain, gzip, BGZF) ->
    ({node: [entry, ...]}, total, totals).  An entry is a dict of taxid, species_taxid, ftp_url, file_name (bytes), quality (the name
    of the AssemblyQuality), is_reference and line; a node is an index into known_taxids; total is the number of records of 20 fields
    and more.  selected: the nodes of the taxfromgenbank set (any iterable of nodes) or None for every node; given and empty, the
    answer is {} and no file is opened, as in the goal.  qualities None allows every quality.  Chunks of whole lines are judged on the
    device, what it refuses by a record-by-record restatement of the reference; GS_HOST_FAST=0 sends everything through the latter.  A
    stop on request raises Cancelled."""
    known = np.ascontiguousarray(known_taxids, dtype=np.int32)
    flt = None
    if selected is not None:
        selected = [int(x) for x in selected]
        if not selected:
            return {}, 0, {f: 0 for f, _ in AsmsumTotals._fields_}
        flt = np.zeros(len(known), dtype=np.uint8)
        flt[np.asarray(selected, dtype=np.int64)] = 1
    cfg = _b.DeviceAssemblySummary.config(known, flt, qualities, reference_only, use_species_taxid)
    paths = [os.fspath(p) for p in paths]
    tot = AsmsumTotals()
    h = C.c_void_p()
    rc = lib().gs_host_asmsum_files(_cstr_array(paths), len(paths), int(device), C.byref(cfg), int(max_per_taxid), C.byref(h), C.byref(tot))
    totals = {f: getattr(tot, f) for f, _ in AsmsumTotals._fields_}
    _check(rc, totals=totals)
    out = {}
    with _b.DeviceAssemblySummary._wrap(h, (totals["kept"], totals["picked"], totals["nodes"], totals["counted"])) as a:
        for node, taxid, species, ftp, quality, is_ref, line in a.fetch():
            out.setdefault(node, []).append({"taxid": taxid, "species_taxid": species, "ftp_url": ftp, "file_name": _b.file_name_of(ftp),
                                             "quality": _b.ASSEMBLY_QUALITIES[quality], "is_reference": is_ref, "line": line})
    return out, totals["counted"], totals


def taxtree_files(nodes_path, names_path=None, device=0):
    """gs_host_taxtree_files: the taxtree goal over nodes.dmp and (unless None) names.dmp, each plain, gzip or BGZF ->
    (DeviceTaxTree, finished; report).  Chunks of whole nodes lines are scanned on the device, what it refuses by a line-by-line
    restatement of the reference; names.dmp goes the same way.  GS_HOST_FAST=0 sends everything through the restatement and
    gives a host-only tree.  A stop on request raises Cancelled: no tree."""
    h = C.c_void_p()
    r = (C.c_int64 * 8)()
    rc = lib().gs_host_taxtree_files(int(device), os.fsencode(nodes_path), os.fsencode(names_path) if names_path is not None else None, C.byref(h), r)
    report = {"nodes_lines": r[0], "names_lines": r[1], "device_chunks": r[2], "host_chunks": r[3], "nodes": r[4], "reached": r[5],
              "duplicates": r[6], "on_host": r[7]}
    _check(rc, report=report)
    return _b.DeviceTaxTree._wrap(h, report), report


def read_taxids_file(path):
    """gs_host_read_taxids_file: a tax id file (plain or gzip) as TaxIdCollector.readFromFile reads it -> (requested, excluded) tax
    ids as int32 arrays, in file order; what is no tax id of 1-9 digits is dropped, as an id that names no node is"""
    cap = os.path.getsize(path) // 2 + 1  # (an id and its newline; an inflated file may hold more: the counts say so)
    while True:
        req, exc = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        n_req, n_exc = C.c_int64(), C.c_int64()
        _check(lib().gs_host_read_taxids_file(os.fsencode(path), req.ctypes.data_as(C.c_void_p), C.byref(n_req), exc.ctypes.data_as(C.c_void_p),
                                              C.byref(n_exc), cap))
        if max(n_req.value, n_exc.value) <= cap:
            return req[:n_req.value], exc[:n_exc.value]
        cap = max(n_req.value, n_exc.value)
