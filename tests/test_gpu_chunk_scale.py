"""The text stages at chunk sizes where their scans change shape.  Every stage finds its offsets with a two-level prefix sum: blocks of
256 items scanned in place, the per-block sums scanned by one block of 1024 threads -- one sum per thread up to 1024 sums, a run of
`per` sums per thread beyond; several kernels also go over to a grid-stride loop once a chunk outgrows their grid.  The workload's
chunks lie far beyond those steps and the shapes of the other test modules in front of them, so here every text is the smallest one
that crosses a step: the four-line cut (gs_text_cut_device) called directly, four-line chunks of more than 262 144 records, FASTA and
general FASTQ of more than 262 144 lines with output beyond the copy grid, text of more than 64 MiB through the record scan, more than
1024 deflate members, and one file of that size through gs_host_extract_files.  The references are those of the other modules
(tests/streamgoals.py, tests/recordtext.py, tests/krakenlines.py, the oracle, zlib, numpy); the texts come from tests/chunkscale.py.
Every test asserts the step it is about on its own input before the device is touched.  Needs an MI355X: run with -m gpu."""
import ctypes as C
import functools
import gzip
import zlib

import numpy as np
import pytest

import chunkscale as cs
import genestrip_amd as ga
import krakenlines
import recordtext as rt
import streamgoals as sg
from conftest import bgzf
from genestrip_amd import host
from oracle import gs_oracle as orc
from test_gpu_deflate import _rewritten
from test_gpu_record_text import _same

pytestmark = pytest.mark.gpu

GS_E_INVALID = -1
TILE = 4096               # GS_TEXT_TILE (gs_text.hip); gi_count_kernel: at = tile * 4096 + threadIdx.x * 16 (gs_inflate_dev.hip)
STEP_TILES = 16 * 1024    # gs_text_scan_kernel and gi_cut_kernel: per = ((n_tiles + 1023) / 1024 + 15) & ~15 -- 16 up to here, 32 beyond
SCAN_ITEMS = 1024 * 256   # per = (n_blocks + 1023) / 1024 over blocks of 256 (GS_SCAN_BLOCK, GS_FA_BLOCK, GC_BLOCK): 1 up to here --
#                           rw_scan_kernel (gs_rewrite.hip), gs_fasta_scan_kernel (gs_text.hip), gc_scan_kernel (gs_deflate_dev.hip)
SCAN_THREADS = 1024       # gd_offsets_kernel: per = (n + 1023) / 1024 members per thread
GATHER_LINES = 8192 * 4   # rw_gather_kernel, gs_fasta_gather_kernel: grid = min((n_lines + 3) / 4, 8192), a wave per line
PIECE = 4096              # RW_PIECE = RW_BLOCK * 16; rw_pieces_kernel: one thread per piece, blocks of RW_BLOCK = 256
TREE3 = np.array([-1, 0, 0], dtype=np.int32)
TAX3 = ["", "5", "1234567"]  # (as tests/test_gpu_kraken_text.py)
assert (TILE, STEP_TILES, SCAN_ITEMS) == (cs.TILE, cs.STEP_TILES, cs.SCAN_THREADS * cs.BLOCK)


def copy_grid(n_cu):
    """gs_launch_rewrite_copy: grid = min(pieces, n_cu * 8) blocks of rw_copy_kernel, a piece of RW_PIECE bytes per block and step"""
    return n_cu * 8 * PIECE


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def reads():
    r = ga.DeviceReads(k=5)
    yield r
    r.close()


@pytest.fixture(scope="module")
def k2():
    d = {}
    for s, vi in (("CC", 0), ("TT", 1), ("AG", 2)):
        d.setdefault(orc.kmer_canonical(s), vi)
    keys = sorted(d)
    s = rt.Side(ga, 2, np.array(keys, dtype=np.int64), np.array([d[x] for x in keys], dtype=np.int32), 3, TREE3)
    yield s
    s.close()


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


# ---- 1. the four-line cut, directly ----
def _on_device(text, off=0):
    """the text at `off` bytes behind the start of a device allocation"""
    import torch
    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if len(text):
        buf[off:off + len(text)] = torch.from_numpy(np.ascontiguousarray(text))
    torch.cuda.synchronize()
    return buf


def _cut(buf, off, n):
    n_lines, cut = C.c_int64(-1), C.c_int64(-1)
    rc = ga.lib().gs_text_cut_device(0, C.c_void_p(buf.data_ptr() + off), n, C.byref(n_lines), C.byref(cut))
    assert rc == 0, ga.lib().gs_inflate_last_error()
    return n_lines.value, cut.value


def test_cut_of_small_texts():
    """lengths around the 16-byte words and the tiles, 0 .. 7 newlines, the target newline at the edges of a tile, of the text and of
    a thread's run of 16 tiles, dense tiles"""
    cases = cs.small_cut_cases()
    want = {name: cs.cut_reference(t) for name, t in cases.items()}
    assert cs.tile_run(40) == 16 and want["target in tile 15 of 40"][1] // TILE == 15 and want["target in tile 16 of 40"][1] // TILE == 16
    assert [want["%d newlines" % k][0] for k in range(8)] == [0, 0, 0, 0, 4, 4, 4, 4]
    for name, t in cases.items():
        buf = _on_device(t)
        assert _cut(buf, 0, len(t)) == want[name], name


def test_cut_at_every_pointer_alignment():
    """gs_host.cpp hands over gz_text + gz_off: the 16-byte loads of gi_count_kernel at any alignment"""
    cases = cs.small_cut_cases()
    for name in ("another count in every tile", "length %d" % (5 * TILE + 1234), "target last byte of the text", "length 17"):
        t = cases[name]
        for off in (0, 1, 7, 15):
            buf = _on_device(t, off)
            assert _cut(buf, off, len(t)) == cs.cut_reference(t), (name, off)


def test_cut_argument_errors():
    lib = ga.lib()
    buf = _on_device(np.frombuffer(bytearray(b"a\nb\nc\nd\n"), dtype=np.uint8))
    p, a, b = C.c_void_p(buf.data_ptr()), C.c_int64(7), C.c_int64(7)
    assert lib.gs_text_cut_device(0, p, 8, None, C.byref(b)) == GS_E_INVALID
    assert lib.gs_text_cut_device(0, p, 8, C.byref(a), None) == GS_E_INVALID
    assert lib.gs_text_cut_device(0, p, -1, C.byref(a), C.byref(b)) == GS_E_INVALID
    assert lib.gs_text_cut_device(0, None, 8, C.byref(a), C.byref(b)) == GS_E_INVALID
    assert (a.value, b.value) == (7, 7)  # (nothing was written)
    assert lib.gs_text_cut_device(0, None, 0, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    assert lib.gs_text_cut_device(0, p, 8, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (4, 8)


@pytest.mark.parametrize("n_tiles", [STEP_TILES, STEP_TILES + 1, STEP_TILES + 16 * 3 + 5])
def test_cut_at_the_tile_step(n_tiles):
    """16 384 tiles: per = 16 and every thread's run full; 16 385: per = 32, thread 512 owns one tile and 511 threads none; 16 437: the
    last run that is not empty is one of 16 counts read as vectors and 5 read one by one"""
    n = cs.step_cut_bytes(n_tiles)
    per = 16 if n_tiles == STEP_TILES else 32
    assert (n + TILE - 1) // TILE == n_tiles and cs.tile_run(n_tiles) == per
    if n_tiles > STEP_TILES:
        assert n > STEP_TILES * TILE and (n_tiles - 1) // per < 1023  # (threads without a tile)
    else:
        assert n == STEP_TILES * TILE and (n_tiles - 1) // per == 1023
    text = np.full(n, ord("A"), dtype=np.uint8)
    for what, pos in cs.step_cut_cases(n_tiles):
        text[pos] = cs.NL
        want = cs.cut_reference(text)
        assert want[0] >= 4 and want[0] == len(pos) & ~3
        buf = _on_device(text)
        assert _cut(buf, 0, n) == want, (what, want)
        del buf
        text[pos] = ord("A")


# ---- 2. four-line chunks beyond 262 144 records ----
@pytest.fixture(scope="module", params=[SCAN_ITEMS + 5, 2 * SCAN_ITEMS + 257], ids=["1025 blocks", "2050 blocks"])
def short(request):
    """the chunk of short records, once per size: the smaller one carries every key and mode, the larger one a single one each"""
    n = request.param
    text, recs, cycle = cs.short_records(n)
    return dict(n=n, text=text, recs=recs, cycle=cycle, ents=rt.entries(text, False), full=n == SCAN_ITEMS + 5)


def _crosses_the_record_step(short):
    n = short["n"]
    n_blocks = (n + 255) // 256
    assert n > SCAN_ITEMS and short["text"].count(b"\n") == 4 * n
    # 1025 blocks: per = 2, thread 512 owns one block, 511 threads none; 2050 blocks: per = 3, the last run (thread 683) holds one block
    assert (n_blocks, (n_blocks + 1023) // 1024, n_blocks % ((n_blocks + 1023) // 1024)) in ((1025, 2, 1), (2050, 3, 1))
    return n


def test_extract_of_short_records(short, reads):
    """gs_reads_select_text + gs_reads_compact_text: gc_len_kernel / gc_scan_kernel / gc_copy_kernel over more than 1024 blocks"""
    n = _crosses_the_record_step(short)
    text, ents = short["text"], short["ents"]
    # a third (sizes of 0 in every block), all, the very last record -- alone in the last block of the larger chunk, the one block of the
    # last run that is not empty, which the key of the third does not take
    keys = {b"s1/": None, b"s": n, b"s-last": 1} if short["full"] else {b"s1/": None, b"s-last": 1}
    wants = {}
    for key, count in keys.items():
        keep = np.array([sg.starts_with(d, key) for d, _, _ in ents])
        assert keep.sum() == (count if count else n // 3) and (count != 1 or keep[-1])
        wants[key] = keep, {p: rt.record_text(ents, keep, p) for p in (True, False)}
    if short["full"]:  # (the goal's own loop, once)
        assert sg.extract(text, b"s1/") == (wants[b"s1/"][1][True], int(wants[b"s1/"][0].sum()))
    for key, (keep, want) in wants.items():
        reads.text_reset(True)
        acc = reads.select_text(text, key)
        assert reads.text_status()[0] == -1 and np.array_equal(acc.astype(bool), keep), key
        for probs in (True, False):
            for slot in (0, 1):
                got, nr = reads.compact_text(with_probs=probs, slot=slot)
                assert nr == keep.sum()
                _same(got, want[probs], f"key {key!r} probs {probs} slot {slot}")


def test_filter_gather_of_short_records(short):
    """gs_filter_submit_text + gs_filter_compact_text: the accepted records and the others partition the chunk"""
    n = _crosses_the_record_step(short)
    text, recs = short["text"], short["recs"]
    keys = np.array(sorted({orc.kmer_canonical(s) for s in ("ACG", "TTT", "CAG", "GGA", "ATC", "CCC")}), dtype=np.int64)
    ob = orc.Bloom(orc.BLOOM_XOR, len(keys), 1e-8)
    ob.put_many(keys)
    seq, off = orc.pack_reads([s for _, s, _, _ in recs])
    want = ob.filter_batch(3, 1, 0.2, seq, off)
    per_block = np.add.reduceat(want.astype(np.int64), np.arange(0, n, 256))
    assert (per_block[:-1] > 0).all() and (per_block[:-1] < 256).all()  # both kinds in every block
    gb = ga.DeviceBloomFilter(ga.BLOOM_XOR, ob.bits, ob.hash_factors, ob.words)
    flt = ga.FastqBloomFilter(3, gb, 1, 0.2)
    acc = np.zeros(n, dtype=np.uint8)
    flt.submit_text(text, acc)
    assert flt.text_status()[0] < 0
    assert np.array_equal(acc, want)
    for probs in (True, False) if short["full"] else (True,):
        got, na = flt.compact_text(1, probs, slot=0)
        assert na == int(want.sum())
        _same(got, _rewritten(recs, want, probs), f"accepted, probs {probs}")
        rest, nr = flt.compact_text(0, probs, slot=1)
        assert nr == n - na
        _same(rest, _rewritten(recs, 1 - want, probs), f"rest, probs {probs}")
    gb.close()


def test_kraken_lines_of_short_records(short, k2):
    """gs_match_kraken_text: kr_size_kernel of the four-line kind and gs_launch_scan_blocks over more than 1024 blocks.  The text,
    the line count, the classes and the segments of the whole chunk are compared; the segments not read by read as
    test_gpu_kraken_text._check_chunk does, but as arrays against one period of the reads repeated (the reads repeat with period
    SHORT_CYCLE)."""
    n = _crosses_the_record_step(short)
    text, cycle = short["text"], short["cycle"]
    cyc_cv, _ = k2.match(cycle, max_paths=4)  # (a read's class depends on the read alone)
    want_cv = np.resize(cyc_cv, n)
    assert 0 < (cyc_cv >= 0).sum() < len(cycle)
    per_read = [k2.segments(r) if len(r) >= 2 else [] for r in cycle]
    assert any(not p for p in per_read) and max(len(p) for p in per_read) > 3
    m = ga.FastqKMerMatcher(k2.store, ga.MatchConfig(max_paths=4))
    m.set_taxids(TAX3)
    for write_all, slot in ((True, 0), (False, 1)) if short["full"] else ((True, 0),):
        lines = krakenlines.chunk_lines(text, 2, k2.segments, want_cv, TAX3, write_all)
        cv, fl = np.full(n, -7, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        m.submit_text(_u8(text), class_vi=cv, flags=fl)
        got = m.kraken_text(write_all, slot)
        assert np.array_equal(cv, want_cv)
        _same(got, b"".join(lines), f"write_all {write_all}")
        assert m.kraken_lines == sum(1 for ln in lines if ln) and 0 < m.kraken_lines < n
    # the segments the call has left for gs_match_segments_fetch
    codes1 = np.array([c for p in per_read for c, _ in p], dtype=np.int32)
    starts1 = np.array([s for p in per_read for s in np.cumsum([0] + [cnt for _, cnt in p[:-1]]).tolist()[:len(p)]], dtype=np.int32)
    q, r = divmod(n, len(cycle))
    head = sum(len(p) for p in per_read[:r])
    codes, starts = m.segments_fetch(q * len(codes1) + head)
    assert np.array_equal(codes, np.concatenate([np.tile(codes1, q), codes1[:head]]))
    assert np.array_equal(starts, np.concatenate([np.tile(starts1, q), starts1[:head]]))
    m.close()


# ---- 3. FASTA and general FASTQ beyond 262 144 lines ----
@pytest.fixture(scope="module")
def fasta(n_cu):
    text = cs.fasta_text(n_cu)
    ents = rt.entries(text, True)
    n_lines = text.count(b"\n")
    # per = 3 in both line scans, per = 2 over the records, the gather kernels in their stride loop
    assert n_lines > 2 * SCAN_ITEMS and (((n_lines + 255) // 256) + 1023) // 1024 == 3 and n_lines > GATHER_LINES
    assert len(ents) > SCAN_ITEMS and (((len(ents) + 255) // 256) + 1023) // 1024 == 2
    long = next(r for d, r, _ in ents if d.startswith(b"@sL "))
    assert len(long) > copy_grid(n_cu) + (1 << 20)  # one record spans the whole copy grid, and more than once with its quality line
    assert max(len(ln) for ln in text.split(b"\n")) + 1 == 60_000 < cs.LONG_LINE
    return text, ents


def test_fasta2fastq_beyond_the_line_step_and_the_copy_grid(fasta, n_cu, reads):
    """gs_reads_fasta2fastq: rw_lines_kernel / rw_scan_kernel / rw_emit_kernel / rw_gather_kernel in goal mode over 3 block sums per
    thread, rw_scan_kernel over the record sizes at 2, rw_pieces_kernel over many blocks, rw_copy_kernel in its grid-stride loop"""
    text, ents = fasta
    want, n_rec = sg.fasta2fastq(text)
    assert n_rec == len(ents) and len(want) > copy_grid(n_cu) and len(want) > 256 * PIECE
    reads.text_reset(True)
    for slot in (0, 1):
        got, long_lines = reads.fasta2fastq(text, slot=slot)
        assert long_lines == 0 and reads.text_status()[0] == -1
        _same(got, want, f"slot {slot}")
    assert reads.text_status()[2][0] == 2 * n_rec


def test_fasta2fastq_with_crlf_and_empty_lines(n_cu, reads):
    """the same text in the shape that needs rw_kept: lines that leave no byte, across the second level of the scan"""
    text = cs.fasta_text(n_cu, crlf=True)
    n_lines = text.count(b"\n")
    assert n_lines > 2 * SCAN_ITEMS and b"\r\n\r\n" in text and b"\n\n" in text and b"\r\r\n" in text
    want, n_rec = sg.fasta2fastq(text)
    assert n_rec > SCAN_ITEMS and len(want) > copy_grid(n_cu)
    reads.text_reset(True)
    got, long_lines = reads.fasta2fastq(text)
    assert long_lines == 0 and reads.text_status()[0] == -1
    _same(got, want, "crlf")


def test_extract_of_fasta_records(fasta, n_cu, reads):
    """gs_reads_select_fasta + gs_reads_compact_text (gs_launch_rewrite_copy): the long record alone, a ninth of the small ones, all"""
    text, ents = fasta
    sizes = {}
    for key in (b"sL", b"s4/", b"s"):
        keep = np.array([sg.starts_with(d, key) for d, _, _ in ents])
        want = rt.record_text(ents, keep, True)
        sizes[key] = int(keep.sum()), len(want)
        if key == b"sL":  # (the goal's own loop, once)
            assert sg.extract(text, key, fasta=True) == (want, 1)
        reads.text_reset(True)
        acc = reads.select_fasta(text, key)
        assert reads.text_status()[0] == -1 and np.array_equal(acc.astype(bool), keep), key
        for slot in (0, 1):
            got, nr = reads.compact_text(slot=slot)
            assert nr == keep.sum()
            _same(got, want, f"key {key!r} slot {slot}")
        if key == b"s4/":
            got, nr = reads.compact_records(True, 0)
            _same(got, want, "compact_records")
    n_small = len(ents) - 2
    assert sizes[b"sL"][0] == 1 and sizes[b"sL"][1] > 2 * copy_grid(n_cu) and sizes[b"s"][0] == len(ents)
    assert abs(sizes[b"s4/"][0] - n_small / 9) <= 2 and sizes[b"s"][1] > 256 * PIECE  # (more than one block of rw_pieces_kernel)


@pytest.fixture(scope="module")
def fasta_match(fasta, k2):
    """the oracle's classes and flags of the FASTA text's records (k = 2 store)"""
    _, ents = fasta
    cv, fl = k2.match([r for _, r, _ in ents], max_paths=4)
    keep = (fl & orc.F_RETURNED) != 0
    assert 0 < keep.sum() < len(ents) and 0 < (cv >= 0).sum() < len(ents)
    return cv, fl, keep


def _submit_fasta(m, text, n):
    cv, fl = np.full(n, -7, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    m.submit_fasta(_u8(text), class_vi=cv, flags=fl)
    return cv, fl


def test_match_records_of_the_fasta_text(fasta, fasta_match, k2):
    """gs_match_submit_fasta + gs_match_compact_records: gs_fasta_scan_kernel at 3 block sums per thread, the record rewrite at 2"""
    text, ents = fasta
    cv_want, fl_want, keep = fasta_match
    want = rt.record_text(ents, keep, False)
    m = ga.FastqKMerMatcher(k2.store, ga.MatchConfig(max_paths=4))
    cv, fl = _submit_fasta(m, text, len(ents))
    for slot in (0, 1):
        got, nr = m.compact_records(False, slot)
        assert nr == keep.sum()
        _same(got, want, f"slot {slot}")
    assert np.array_equal(cv, cv_want) and np.array_equal(fl, fl_want)
    m.close()


@pytest.mark.parametrize("write_all", [True, False])
def test_kraken_lines_of_the_fasta_text(fasta, fasta_match, k2, write_all):
    """gs_match_kraken_records: kr_size_kernel of the record kind and gs_launch_scan_blocks over more than 1024 blocks"""
    text, ents = fasta
    cv_want, _, _ = fasta_match
    want = rt.kraken_text(ents, 2, k2.segments, cv_want, TAX3, write_all)
    m = ga.FastqKMerMatcher(k2.store, ga.MatchConfig(max_paths=4))
    m.set_taxids(TAX3)
    cv, _ = _submit_fasta(m, text, len(ents))
    got = m.kraken_records(write_all, int(not write_all))
    assert np.array_equal(cv, cv_want)
    _same(got, want, f"write_all {write_all}")
    assert m.kraken_lines == want.count(b"\n") > 0
    m.close()


@pytest.fixture(scope="module")
def fastq_ml():
    recs = cs.fastq_ml_records(60_000)
    text = rt.fastq_ml(recs)
    ents = rt.entries(text, False)
    n_lines = text.count(b"\n")
    assert n_lines >= 270_000 > SCAN_ITEMS and (((n_lines + 255) // 256) + 1023) // 1024 == 2 and len(ents) == len(recs)
    assert any(len(q) > len(r) for _, r, q in ents)
    half = b"@K1/half ml\nACGTACGTAC\nGTAC\n"  # the sequence lines of one more record, no '+' line yet
    return text, ents, half


def test_select_general_fastq_beyond_the_line_step(fastq_ml, reads):
    """gs_reads_select_fastq_ml + gs_reads_compact_records; the chunk ends in the middle of a record once"""
    text, ents, half = fastq_ml
    keep = np.array([sg.starts_with(d, b"K1/") for d, _, _ in ents])
    assert abs(3 * int(keep.sum()) - len(ents)) <= 3
    for tail in (half, b""):
        reads.text_reset(True)
        n_rec, used, acc = reads.select_fastq_ml(text + tail, b"K1/")
        assert (n_rec, used) == (len(ents), len(text)) and reads.text_status()[0] == -1
        assert np.array_equal(acc.astype(bool), keep)
        for probs, slot in ((True, 0), (False, 1)):
            got, nr = reads.compact_records(probs, slot)
            assert nr == keep.sum()
            _same(got, rt.record_text(ents, keep, probs), f"probs {probs}")


def test_match_records_of_general_fastq_in_quality_mode(fastq_ml, k2):
    """gs_match_submit_fastq_ml + gs_match_compact_records(with_probs): rw_lines_kernel in goal_mode 2 over more than 1024 blocks"""
    text, ents, half = fastq_ml
    cv_want, fl_want = k2.match([r for _, r, _ in ents], max_paths=4)
    keep = (fl_want & orc.F_RETURNED) != 0
    per_block = np.add.reduceat(keep.astype(np.int64), np.arange(0, len(ents), 256))
    assert (per_block[:-1] > 0).all() and (per_block[:-1] < 256).all()
    m = ga.FastqKMerMatcher(k2.store, ga.MatchConfig(max_paths=4))
    room = (text + half).count(b"\n") // 4 + 2
    cv, fl = np.full(room, -7, dtype=np.int32), np.zeros(room, dtype=np.uint8)
    n_rec, used = m.submit_fastq_ml(_u8(text + half), class_vi=cv, flags=fl)
    assert (n_rec, used) == (len(ents), len(text))
    for probs, slot in ((True, 0), (False, 1)):
        got, nr = m.compact_records(probs, slot)
        assert nr == keep.sum()
        _same(got, rt.record_text(ents, keep, probs), f"probs {probs}")
    assert np.array_equal(cv[:n_rec], cv_want) and np.array_equal(fl[:n_rec], fl_want)
    m.close()


# ---- 4. text beyond 64 MiB through the record scan ----
@functools.lru_cache(maxsize=None)
def wide_text(n_tiles):
    text = cs.wide_chunk(n_tiles * TILE - 1000)
    assert (len(text) + TILE - 1) // TILE == n_tiles
    return text


@pytest.mark.parametrize("n_tiles", [STEP_TILES, STEP_TILES + 1, STEP_TILES + 16 * 3 + 5])
def test_extract_of_a_chunk_at_the_tile_step(n_tiles, reads):
    """gs_text_scan_kernel at per = 16 with every run full, at per = 32 with one tile in the last run, and with 16 + 5: any slip in
    the tile prefix moves nl[] and with it every record behind"""
    text = wide_text(n_tiles)
    if n_tiles > STEP_TILES:
        assert len(text) > STEP_TILES * TILE and cs.tile_run(n_tiles) == 32
    else:
        assert len(text) > (STEP_TILES - 1) * TILE and cs.tile_run(n_tiles) == 16
    counts = cs.tile_counts(text)
    assert (np.add.reduceat(counts, np.arange(0, n_tiles, 16)) > 0).all() and counts.max() > 500 and (counts == 0).any()
    want, n = sg.extract(text, b"w1/")
    n_recs = text.count(b"\n") // 4
    assert abs(3 * n - n_recs) <= 3
    reads.text_reset(True)
    acc = reads.select_text(text, b"w1/")
    assert reads.text_status()[0] == -1 and int(acc.sum()) == n and len(acc) == n_recs
    got, nr = reads.compact_text(with_probs=True, slot=0)
    assert nr == n
    _same(got, want, "with qualities")
    got, nr = reads.compact_text(with_probs=False, slot=1)
    assert nr == n
    _same(got, sg.extract(text, b"w1/", with_probs=False)[0], "without qualities")


def test_a_wrong_line_count_is_refused_at_that_size(reads):
    text = wide_text(STEP_TILES + 1)
    assert len(text) > STEP_TILES * TILE
    t, key = _u8(text), _u8(b"w1/")
    n_lines = text.count(b"\n")
    acc = np.zeros(n_lines // 4, dtype=np.uint8)
    reads.text_reset(True)
    ga.binding._check(ga.lib().gs_reads_select_text(reads.h, reads.k, ga.binding._ptr(t)[0], len(t), n_lines - 4, ga.binding.MEM_HOST,
                                                    ga.binding._ptr(key)[0], len(key), ga.binding._ptr(acc)[0], None, None))
    failed, _, totals = reads.text_status()
    assert failed >= 0 and totals[0] == 0 and int(acc.sum()) == 0
    try:
        got, nr = reads.compact_text()
    except ga.GsError:
        got, nr = b"", 0
    assert (len(got), nr) == (0, 0)
    reads.text_reset(True)
    assert int(reads.select_text(text[:text.index(b"\n@w1/") + 1], b"w0/").sum()) == 1  # (the handle works on)


# ---- 5. more than 1024 deflate members ----
@pytest.mark.parametrize("n_pieces", [1025, 2049])
def test_deflate_offsets_beyond_1024_members(monkeypatch, n_pieces):
    """gd_offsets_kernel at 2 and 3 members per thread (1026 and 2050 members: the last one holds the odd bytes)"""
    piece = 16384  # GD_PIECE_MIN
    monkeypatch.setenv("GS_DEFLATE_PIECE", str(piece))
    data = cs.deflate_text(n_pieces * piece + (1 if n_pieces == 1025 else 7))
    n_members = (len(data) + piece - 1) // piece
    assert n_members == n_pieces + 1 > SCAN_THREADS and (n_members + 1023) // 1024 == (2 if n_pieces == 1025 else 3)
    comp = ga.deflate_device(data).tobytes()
    members, reached = ga.bgzf_members(comp)
    assert reached == len(comp) and len(members) == n_members
    at = 0
    sizes = []
    for po, pl, isz, crc in members:
        text = zlib.decompress(comp[po:po + pl], -15)
        assert len(text) == isz == min(piece, len(data) - at) and zlib.crc32(text) == crc and text == data[at:at + isz], at
        at += isz
        sizes.append(pl)
    assert at == len(data) and max(sizes) > 2 * min(sizes[:-1])  # (sizes that differ widely: an offset that slips lands inside a member)
    assert gzip.decompress(comp + ga.BGZF_EOF) == data
    text, status = ga.inflate_members(comp, members)
    assert not status.any() and text.tobytes() == data


# ---- 6. file level, once ----
@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
def test_extract_of_a_file_beyond_the_tile_step(tmp_path, kind):
    """gs_host_extract_files on one file of 16 385 tiles and a last record without its newline.  bgzf: one feed of the inflater --
    its own cut launch (gi_cut_kernel at per = 32) and the record scan at per = 32 in place; gzip: the slices of a single-member
    stream, cut by gs_text_cut_device wherever the slice before ended.  (The last record is one the key does not take: the reader
    restated in tests/streamgoals.py is for whole records, and the reference's own shortens a last quality line without a newline --
    tests/test_gpu_host.py has that shape.  It counts as a read, and the cut has to step back in front of it.)"""
    text = wide_text(STEP_TILES + 1) + b"@w0/cut lane\nACGT\n+\nIIII"
    assert len(text) > STEP_TILES * TILE and text.count(b"\n") % 4 == 3
    want, n = sg.extract(text, b"w1/")
    assert want == sg.extract(wide_text(STEP_TILES + 1), b"w1/")[0] and abs(3 * n - text.count(b"\n") // 4) <= 3
    src = tmp_path / "wide.fastq.gz"
    src.write_bytes(bgzf(text, level=1) if kind == "bgzf" else gzip.compress(text, 1))
    dst = tmp_path / "out.fastq"
    tot = host.extract_files(b"w1/", [src], dst, k=31)
    assert tot.filtered_reads == n and tot.reads == text.count(b"\n") // 4 + 1
    _same(dst.read_bytes(), want, kind)
