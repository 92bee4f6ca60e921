"""gs_genomes (genome FASTA text -> the regions of the kept records, gs_genomes.hip) against tests/genomefasta.py, byte for byte:
header lines, bases, offsets, the longest line, the records that end in the chunk and the bytes they cover.  The shapes are the
smallest at which a mechanism of the kernels changes: a thread owns 16 bytes and a block one tile of 4096, the gather stores 16
bytes at once where they are 16 bases of one record, the scans over tiles and over records go through a second level from 1025
block sums on, and the look-ahead behind a '\\r' is capped at 64.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import chunkscale as cs
import genestrip_amd as ga
import genomefasta as gf
from genomefasta_cases import CASES

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE = -4, -5
TILE = 4096   # GS_GN_TILE: the piece of the gather
CR_CAP = 64   # GS_GN_CR_CAP
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def _want(data, last=True, keep=None):
    headers, seq, offsets, max_line, consumed = gf.read_fasta(data, last)
    if keep is None:
        keep = np.ones(len(headers), dtype=bool)
    parts = [seq[offsets[i]:offsets[i + 1]] for i in range(len(headers)) if keep[i]]
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
    return headers, b"".join(parts), off, max_line, consumed


def _got(g, data, last=True, keep=None, device=False):
    text = np.frombuffer(data, dtype=np.uint8)
    if device:
        import torch
        text = torch.from_numpy(text.copy()).cuda()
    n_records, consumed, header_bytes, max_line = g.scan(text, last)
    hdr, hoff = g.headers()
    assert len(hoff) == n_records + 1 and hoff[0] == 0 and int(hoff[-1]) == header_bytes == len(hdr)
    headers = [hdr[int(hoff[i]):int(hoff[i + 1])].tobytes() for i in range(n_records)]
    n_regions, n_bases = g.gather(keep)
    seq, off = g.regions()
    off = off.numpy()
    assert len(off) == n_regions + 1 and int(off[-1]) == n_bases
    return headers, seq.numpy().tobytes(), off, max_line, consumed


def _same(g, data, last=True, keep=None, device=False):
    got, want = _got(g, data, last, keep, device), _want(data, last, keep)
    assert got[0] == want[0]
    assert got[4] == want[4] and got[3] == want[3]
    assert np.array_equal(got[2], want[2])
    assert got[1] == want[1]
    return want


@pytest.fixture(scope="module")
def g():
    h = ga.DeviceGenomes()
    yield h
    h.close()


@pytest.mark.parametrize("case", [c for c in CASES if b"\x00" not in c[1]], ids=[c[0] for c in CASES if b"\x00" not in c[1]])
def test_hand_written_streams(g, case):
    _, data, last, headers, seq, offsets, max_line, consumed = case
    got = _got(g, data, last)
    assert got[0] == headers and got[1] == seq and list(got[2]) == offsets and got[3:] == (max_line, consumed)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["LF", "CRLF"])
def test_line_lengths_around_a_thread_and_a_wave(g, eol):
    """lines of 0 .. 65 bases behind headers of 1 .. 17 bytes: every line length starts at every offset inside a thread's 16 bytes"""
    rng = np.random.default_rng(1)
    recs = []
    for hl in range(1, 18):
        for L in (0, 1, 15, 16, 17, 63, 64, 65):
            recs.append(b">" + b"h" * (hl - 1) + eol + b"".join(_bases(rng, L) + eol for _ in range(3)))
    data = b"".join(recs)
    want = _same(g, data)
    assert len(want[0]) == 17 * 8 and len(want[1]) == 17 * 3 * (1 + 15 + 16 + 17 + 63 + 64 + 65)
    _same(g, data, keep=np.arange(17 * 8) % 3 != 1)


@pytest.mark.parametrize("src,dst", [(0, 5), (3, 0), (7, 11), (0, 0)], ids=["destination", "source", "both", "neither"])
def test_sixteen_byte_stores_unaligned_at_source_and_destination(g, src, dst):
    """the bases of the second record start at byte = src (mod 16) of the text and go to byte = dst (mod 16) of seq"""
    rng = np.random.default_rng(2)
    first = b">p\n" + _bases(rng, 16 + dst) + b"\n"
    pad = (src - (len(first) + 2)) % 16
    data = first + b">" + b"x" * pad + b"\n" + _bases(rng, 333) + b"\n"
    assert data.index(b"\n", len(first)) + 1 & 15 == src
    want = _same(g, data)
    assert int(want[2][1]) & 15 == dst


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 70001], ids=["piece-1", "piece", "piece+1", "above 65536"])
def test_unwrapped_records(g, n):
    """one line per record, of one piece of the gather less one byte, one piece, one more, and more than 65 536 bytes (where the
    reference's line buffer ends: reported as max_line_bytes, not refused)"""
    rng = np.random.default_rng(3)
    data = b"".join(b">u%d\n" % i + _bases(rng, n - 1) + b"\n" for i in range(3)) + b">tail\n" + _bases(rng, n - 1)
    want = _same(g, data)
    assert want[3] == n and len(want[1]) == 4 * (n - 1)
    _same(g, data, keep=[0, 1, 0, 1])
    _same(g, data[:-5], last=False)


def _mixed(rng, n_records, crlf_every=3):
    recs = []
    for i in range(n_records):
        eol = b"\r\n" if i % crlf_every == 0 else b"\n"
        n = int(rng.integers(0, 400)) if i % 7 else 0
        w = int(rng.choice([1, 15, 16, 17, 60, 70, 80, 1000]))
        body = _bases(rng, n)
        recs.append(b">r%d some text %s" % (i, b"y" * (i % 23)) + eol + b"".join(body[j:j + w] + eol for j in range(0, n, w)) + (b"\n" if i % 5 == 2 else b""))
    return recs


def test_tile_scan_beyond_one_sum_per_thread(g):
    """more than 1024 tiles: a thread of the scan over the per-tile sums owns a run of them"""
    rng = np.random.default_rng(4)
    line = lambda: _bases(rng, 60) + b"\n"
    recs = [b">c%d\n" % i + b"".join(line() for _ in range(int(rng.integers(100, 260)))) for i in range(400)]
    data = b"".join(recs)
    assert cs.tiles(len(data)) > cs.SCAN_THREADS and cs.block_run(cs.tiles(len(data)) * cs.BLOCK) == 2
    _same(g, data)
    _same(g, data, keep=np.arange(400) % 10 == 3)
    _same(g, data[:-1000], last=False, keep=np.arange(399) % 2 == 0)


def test_record_scans_beyond_one_sum_per_thread(g):
    """more than 262 144 records: the scans over the records (header offsets, the kept records' bases) take their second level"""
    n = cs.BLOCK * cs.SCAN_THREADS + 700
    assert cs.block_run(n) == 2
    pool = [b">\nA\n", b">ab\n", b">x\nAC\nG\n", b">yy\r\nT\r\n"]
    data = b"".join(pool[(i * 7 + i // 5) % 4] for i in range(n))
    _same(g, data)
    _same(g, data, keep=np.arange(n) % 2 == 0)


KEEPS = {"all": lambda n: np.ones(n, bool), "none": lambda n: np.zeros(n, bool), "alternating": lambda n: np.arange(n) % 2 == 1,
         "only the first": lambda n: np.arange(n) == 0, "only the last": lambda n: np.arange(n) == n - 1}


@pytest.mark.parametrize("which", sorted(KEEPS))
def test_keep_flags(g, which):
    data = b"".join(_mixed(np.random.default_rng(5), 41))
    keep = KEEPS[which](41)
    want = _same(g, data, keep=keep)
    assert len(want[2]) == int(keep.sum()) + 1


def test_keep_none_is_every_record_and_a_second_gather_replaces_the_first(g):
    data = b"".join(_mixed(np.random.default_rng(6), 30))
    all_ = _same(g, data, keep=None)
    g.gather(np.arange(30) % 3 == 0)
    seq, off = g.regions()
    want = _want(data, True, np.arange(30) % 3 == 0)
    assert seq.numpy().tobytes() == want[1] and np.array_equal(off.numpy(), want[2]) and len(want[1]) < len(all_[1])


def test_empty_record_kept_between_two_long_ones(g):
    rng = np.random.default_rng(7)
    data = b">long one\n" + _bases(rng, 3 * TILE + 5) + b"\n>empty\n>long two\n" + _bases(rng, 2 * TILE + 9) + b"\n"
    want = _same(g, data)
    assert list(np.diff(want[2].astype(np.int64))) == [3 * TILE + 5, 0, 2 * TILE + 9]
    _same(g, data, keep=[0, 1, 1])
    _same(g, data, keep=[0, 1, 0])


@pytest.mark.parametrize("edge", [16, TILE, 2 * TILE])
def test_terminators_and_headers_across_thread_and_tile_edges(g, edge):
    """a '\\r' in the last byte of a thread's 16 and of a tile, with its '\\n' or with a base in the first byte of the next; a header
    line that starts there; a '\\r' run that straddles the edge"""
    rng = np.random.default_rng(8)
    head = b">e\n"
    fill = lambda n: _bases(rng, n)
    for tail in (b"\r\nAC\n", b"\rC\nAC\n", b"\n>next\nAC\n", b"\r\r\r\nAC\n", b"\r\r\rG\n"):
        for shift in (0, 1, 2):
            data = head + fill(edge - len(head) - 1 + shift - 1) + tail + b">z\n" + fill(40) + b"\r"
            _same(g, data)


@pytest.mark.parametrize("where", ["inside a header line", "inside a data line", "behind a newline"])
def test_chunk_that_does_not_end_the_stream(g, where):
    rng = np.random.default_rng(9)
    recs = _mixed(rng, 19, crlf_every=4) + [b">the last one\n" + _bases(rng, 50) + b"\n" + _bases(rng, 30) + b"\n"]
    data = b"".join(recs)
    last_start = len(data) - len(recs[-1])
    cut = {"inside a header line": last_start + 4, "inside a data line": len(data) - 7, "behind a newline": len(data)}[where]
    assert where != "behind a newline" or data.endswith(b"\n")
    want = _same(g, data[:cut], last=False)
    assert want[4] == last_start and len(want[0]) == 19
    _same(g, data[:cut], last=False, keep=np.arange(19) % 2 == 0)
    # ... and the rest in front of what follows gives the last record
    rest = _same(g, data[want[4]:], last=True)
    assert len(rest[0]) == 1


def test_last_chunk_without_a_final_newline(g):
    rng = np.random.default_rng(10)
    data = b"".join(_mixed(rng, 9)) + b">fin\n" + _bases(rng, 100) + b"\n" + _bases(rng, 37)
    want = _same(g, data)
    assert want[1].endswith(data[-37:])
    _same(g, data + b"\r")
    _same(g, data + b"\r\r")


def test_no_header_line_at_all(g):
    data = b"ACGT\nAC\r\nGGG"
    assert _same(g, data, last=False)[4] == 9
    assert _same(g, data, last=True)[4] == len(data)
    assert _got(g, b"", last=True) == ([], b"", _want(b"")[2], 0, 0)


def test_refused_chunks_leave_the_handle_usable(g):
    rng = np.random.default_rng(12)
    good = b"".join(_mixed(rng, 12))
    nul = good[:1000] + b"\x00" + good[1000:] + b"\x00"
    with pytest.raises(ga.GsError) as e:
        g.scan(nul)
    assert e.value.code == UNSUPPORTED and "NUL" in str(e.value) and "offset 1000" in str(e.value)
    for call in (g.headers, g.gather, g.regions):
        with pytest.raises(ga.GsError) as e2:
            call()
        assert e2.value.code == STATE
    _same(g, good)

    at_cap = b">c\nAC" + b"\r" * CR_CAP + b"GT\n" + b"AA" + b"\r" * CR_CAP + b"\n>d\nTT" + b"\r" * CR_CAP
    want = _same(g, at_cap)
    assert want[1] == b"AC" + b"\r" * CR_CAP + b"GTAATT"
    for k, over in enumerate((b">c\nAC" + b"\r" * (CR_CAP + 1) + b"GT\n", b">c\nAC\n" + b"A" * 4000 + b"\r" * (CR_CAP + 1) + b"\n>d\n")):
        with pytest.raises(ga.GsError) as e:
            g.scan(over)
        assert e.value.code == UNSUPPORTED and "'\\r'" in str(e.value) and "offset %d" % over.index(b"\r") in str(e.value), k
        _same(g, good, keep=np.arange(12) % 2 == 0)


def test_chunk_of_two_to_the_24_header_lines_is_refused(g):
    """the selection scan keeps the kept records in 24 bits: 2^24 - 1 header lines are taken (and counted right), 2^24 are refused
    before anything is selected, and the handle takes the next chunk"""
    limit = 1 << 24
    text = np.tile(np.frombuffer(b">\n", dtype=np.uint8), limit)
    n_records, consumed, header_bytes, max_line = g.scan(text[:-2], True)
    assert (n_records, consumed, header_bytes, max_line) == (limit - 1, 2 * limit - 2, limit - 1, 2)
    assert g.gather(None) == (limit - 1, 0)
    keep = np.arange(limit - 1) % 2 == 0
    assert g.gather(keep) == (limit // 2, 0)
    off = g.regions()[1].numpy()
    assert len(off) == limit // 2 + 1 and not off.any()
    with pytest.raises(ga.GsError) as e:
        g.scan(text, True)
    assert e.value.code == UNSUPPORTED and str(limit) in str(e.value) and "header lines" in str(e.value)
    with pytest.raises(ga.GsError) as e2:
        g.gather()
    assert e2.value.code == STATE
    _same(g, b">a\nACGT\n>b\nGG\n")


def test_host_text_and_device_text_agree(g):
    import torch
    data = b"".join(_mixed(np.random.default_rng(13), 25))
    host = _same(g, data)
    dev = _same(g, data, device=True)
    assert host[1] == dev[1]
    # a device text that does not start on a 16-byte boundary
    t = torch.from_numpy(np.frombuffer(b"#" + data, dtype=np.uint8).copy()).cuda()[1:]
    n_records, consumed, _, _ = g.scan(t, True)
    assert (n_records, consumed) == (25, len(data))
    g.gather()
    assert g.regions()[0].numpy().tobytes() == host[1]


def test_call_order_and_kernel_time():
    h = ga.DeviceGenomes()
    for call in (h.headers, h.gather, h.regions):
        with pytest.raises(ga.GsError) as e:
            call()
        assert e.value.code == STATE
    h.scan(b">a\nACGT\n")
    with pytest.raises(ga.GsError) as e:
        h.regions()
    assert e.value.code == STATE
    h.gather()
    assert h.regions()[0].numpy().tobytes() == b"ACGT"
    ms_scan, ms_gather = h.kernel_time()
    assert ms_scan > 0 and ms_gather > 0
    with pytest.raises(ga.GsError) as e:
        h.scan(np.zeros((1 << 30) + 1, dtype=np.uint8))
    assert e.value.code == UNSUPPORTED
    h.close()


def test_regions_feed_the_builder_from_device_memory(g):
    """the regions go into gs_dbbuild_add as they are, and give the k-mers of the same regions from host memory"""
    rng = np.random.default_rng(14)
    data = b"".join(b">g%d\n" % i + b"".join(_bases(rng, 70) + b"\n" for _ in range(9)) for i in range(6))
    keep = np.array([1, 0, 1, 1, 0, 1], bool)
    want = _same(g, data, keep=keep)
    parent = np.array([-1, 0, 0, 0, 0], np.int32)
    nodes = np.array([1, 2, 3, 4], np.int32)
    out = []
    for regions in (g.regions(), (np.frombuffer(want[1], np.uint8), want[2])):
        b = ga.DeviceDbBuilder(31, 5, parent)
        b.add(regions[0], regions[1], nodes)
        out.append(b.finish())
        b.close()
    assert len(out[0][0]) > 2000 and np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
