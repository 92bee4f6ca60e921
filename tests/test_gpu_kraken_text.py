"""gs_match_kraken_text: the Kraken-style lines of a four-line chunk, written on the device, byte for byte against the plain-Python
rule of tests/krakenlines.py over the oracle's classes and segments -- at every segment count where the text kernels change their
way (one thread per line, the wave-wide sizing, the block-wide long line), at every digit boundary of the counts and of L, for the
descriptor rule, the taxid strings, the selection, chunk sizes around the blocks of 256 reads, both slots and every state error.
Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import genestrip_amd as ga
import krakenlines
import matchcheck
from genestrip_amd import synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

GS_E_INVALID, GS_E_STATE = -1, -5
TREE3 = np.array([-1, 0, 0], dtype=np.int32)
TAX3 = ["", "5", "1234567"]  # lengths 0, 1 and 7


class Side:
    """a store on the device, the same store in the oracle, and the oracle's segments per distinct read"""

    def __init__(self, k, kmers, vidx, n_values, parent):
        self.k = k
        self.store = ga.DeviceKMerStore(k, kmers, vidx, n_values, parent)
        self.odb = orc.DB(k, kmers, vidx, n_values, parent)
        self._segs = {}

    def segments(self, read):
        read = bytes(read)
        if read not in self._segs:
            self._segs[read] = self.odb.segments(read, cap=max(4096, len(read) + 1))
        return self._segs[read]

    def classes(self, text, **cfg):
        seq, off = orc.pack_reads([s for _, s in krakenlines.records(text)])
        return matchcheck.oracle_batch(self.odb, seq, off, **cfg)["class_vi"]

    def close(self):
        self.store.close()


@pytest.fixture(scope="module")
def k2():
    d = {}
    for s, vi in (("CC", 0), ("TT", 1), ("AG", 2)):
        d.setdefault(orc.kmer_canonical(s), vi)
    keys = sorted(d)
    s = Side(2, np.array(keys, dtype=np.int64), np.array([d[x] for x in keys], dtype=np.int32), 3, TREE3)
    yield s
    s.close()


@pytest.fixture(scope="module")
def sdb():
    return synth.SynthDB(genera=3, species_per_genus=3, genome_len=20000, seed=11)


@pytest.fixture(scope="module")
def k31(sdb):
    s = Side(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    yield s
    s.close()


def _text(recs, crlf=False):
    nl = b"\r\n" if crlf else b"\n"
    return b"".join(d + nl + r + nl + b"+" + nl + b"I" * len(r) + nl for d, r in recs)


def _submit(m, text):
    n = text.count(b"\n") // 4
    cv = np.full(max(n, 1), -7, dtype=np.int32)
    fl = np.zeros(max(n, 1), dtype=np.uint8)
    m.submit_text(np.frombuffer(text, dtype=np.uint8), class_vi=cv, flags=fl)
    return cv[:n]


def _check_chunk(side, m, text, taxids, write_all=True, slot=0, classes=None, segments=True, **cfg):
    """one chunk through the device and through the rule; returns the device's text"""
    want_cv = side.classes(text, **cfg) if classes is None else classes
    want = krakenlines.chunk_lines(text, side.k, side.segments, want_cv, taxids, write_all)
    cv = _submit(m, text)
    got = m.kraken_text(write_all, slot)
    assert np.array_equal(cv, want_cv), f"classes differ at reads {np.flatnonzero(cv != want_cv)[:8].tolist()}"
    if got != b"".join(want):
        glines = got.split(b"\n")
        wlines = b"".join(want).split(b"\n")
        for i, (a, b) in enumerate(zip(glines, wlines)):
            assert a == b, f"line {i}: device {a[:200]!r} rule {b[:200]!r}"
        raise AssertionError(f"device text {len(got)} bytes, rule {len(b''.join(want))} bytes")
    assert m.kraken_lines == sum(1 for w in want if w)
    if segments:  # the call has left this chunk's segments where gs_match_segments_fetch finds them
        recs = krakenlines.records(text)
        per_read = [side.segments(s) if len(s) >= side.k else [] for _, s in recs]
        codes, starts = m.segments_fetch(sum(len(p) for p in per_read))
        at = 0
        for r, ((_, s), p) in enumerate(zip(recs, per_read)):
            c, st = codes[at:at + len(p)].tolist(), starts[at:at + len(p)].tolist()
            cnt = [b - a for a, b in zip(st, st[1:] + [len(s) - side.k + 1])]
            assert list(zip(c, cnt)) == p, f"segments of read {r} differ"
            at += len(p)
    return got


def test_segment_counts_at_every_wave_and_tile_boundary(k2):
    rng = np.random.default_rng(4)
    want = {1, 2, 63, 64, 65, 127, 128, 129}
    seen, big, reads = set(), False, []
    while (want - seen or not big) and len(reads) < 6000:
        r = bytes(b"ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(3, 401))))
        n = len(k2.segments(r))
        seen.add(n)
        big = big or n >= 250
        reads.append(r)
    assert not (want - seen) and big, (want - seen, max(seen))  # (before the device is touched)
    reads.insert(len(reads) // 2, b"C")  # one base: no segment, no line
    text = _text([(b"@r%d extra" % i, r) for i, r in enumerate(reads)])
    m = ga.FastqKMerMatcher(k2.store, ga.MatchConfig(max_paths=4))
    m.set_taxids(TAX3)
    a = _check_chunk(k2, m, text, TAX3, True, max_paths=4)
    b = _check_chunk(k2, m, text, TAX3, False, max_paths=4)
    assert len(b) < len(a)
    other = ["99", "", "x" * 40]  # a second set replaces the first: the same chunk again
    m.set_taxids(other)
    _check_chunk(k2, m, text, other, True, max_paths=4)
    m.close()


def test_digit_boundaries_bad_base_and_a_record_of_pieces(sdb, k31):
    g = sdb.genomes
    recs = []
    for n in (39, 40, 129, 130, 1029, 1030, 10029):  # runs of 9 .. 9 999 equal k-mers, L of 2 .. 5 digits
        recs.append((b"@slice%d" % n, bytes(g[0, :n])))
        assert [c for _, c in k31.segments(recs[-1][1])] == [n - 30]  # (one run: checked before the device is touched)
    bad = bytearray(g[2, 500:700])
    bad[90] = ord("N")  # an 'A' segment of 31 windows in the middle
    recs.append((b"@withN", bytes(bad)))
    recs.append((b"@long", bytes(g[3]) + bytes(g[4, :13000])))  # 33 000 bases: the segments come in pieces
    assert len(recs[-1][1]) == 33000
    text = _text(recs)
    m = ga.FastqKMerMatcher(k31.store)
    m.set_taxids(sdb.taxids)
    got = _check_chunk(k31, m, text, sdb.taxids)
    assert b":9 " in got or b":9\n" in got
    assert b":9999" in got and b"A:31" in got and b"\t10029\t" in got and b"\t33000\t" in got
    m.close()


def test_descriptors(sdb, k31):
    seq, off = synth.reads_host(sdb.genomes, 16, seed=5)
    read = lambda i: bytes(seq[int(off[i]):int(off[i + 1])])
    descs = [b"@", b"@ x", b"@name", b"@name ", b"@a b c", b"@" + b"n" * 63, b"@" + b"m" * 64 + b" d", b"@" + b"o" * 65, b"@" + b"p" * 300 + b" tail",
             b"@ta\tb x", b"@b\xc3\xa4r\xff y", b"", b" lead", b"@" + b"q" * 5000]
    recs = [(d, read(i)) for i, d in enumerate(descs)]
    m = ga.FastqKMerMatcher(k31.store)
    m.set_taxids(sdb.taxids)
    got = _check_chunk(k31, m, _text(recs), sdb.taxids)
    assert b"\tta\tb\t" in got and b"\tb\xc3\xa4r\xff\t" in got and b"q" * 5000 in got
    # CRLF: the '\r' ends the name when there is no blank, counts into L, and makes the last window 'A'
    got = _check_chunk(k31, m, _text(recs[:6], crlf=True), sdb.taxids)
    assert b"\tname\r\t" in got and b"\t151\t" in got and got.count(b" A:1\n") == 6
    m.close()


def test_selection(sdb, k31):
    seq, off = synth.reads_host(sdb.genomes, 300, seed=9)
    rng = np.random.default_rng(1)
    recs = []
    for i in range(300):
        r = bytes(seq[int(off[i]):int(off[i + 1])])
        if i % 3 == 0:
            r = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 150))  # no hit: not classified
        recs.append((b"@s%d" % i, r))
    text = _text(recs)
    for classify in (True, False):
        m = ga.FastqKMerMatcher(k31.store, ga.MatchConfig(classify=classify))
        m.set_taxids(sdb.taxids)
        a = _check_chunk(k31, m, text, sdb.taxids, True, classify=classify)
        b = _check_chunk(k31, m, text, sdb.taxids, False, classify=classify)
        assert a.count(b"\n") == 300
        if classify:
            assert 0 < b.count(b"\n") < 300 and a.count(b"U\t") == 300 - b.count(b"\n")
        else:  # a run that does not classify: every line 'U', none without write_all
            assert b == b"" and a.count(b"U\t") == 300
        # a chunk in which no read prints a line
        short = _text([(b"@t%d" % i, b"ACGT" * 5) for i in range(300)])
        assert _check_chunk(k31, m, short, sdb.taxids, True, classify=classify) == b"" and m.kraken_lines == 0
        m.close()


@pytest.fixture(scope="module")
def cycle(sdb, k31):
    """a few hundred distinct reads, their classes and their lines (computed once)"""
    seq, off = synth.reads_host(sdb.genomes, 300, seed=21)
    recs = [(b"@q" + b"x" * (j % 13) + b"%d rest" % j, bytes(seq[int(off[j]):int(off[j + 1])])) for j in range(300)]
    recs[7] = (recs[7][0], recs[7][1][:60] + b"N" + recs[7][1][61:])
    text = _text(recs)
    cv = k31.classes(text)
    return recs, cv, krakenlines.chunk_lines(text, 31, k31.segments, cv, sdb.taxids, True)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025, 70001])
def test_chunk_sizes(sdb, k31, cycle, n):
    recs, cv, lines = cycle
    text = _text([recs[i % 300] for i in range(n)])
    m = ga.FastqKMerMatcher(k31.store)
    m.set_taxids(sdb.taxids)
    got_cv = _submit(m, text)
    got = m.kraken_text(True, 0)
    assert np.array_equal(got_cv, np.resize(cv, n))
    assert got == b"".join(lines[i % 300] for i in range(n))
    assert m.kraken_lines == n
    m.close()


def test_slots_alternate_and_keep_their_text(sdb, k31, cycle):
    recs, cv, lines = cycle
    m = ga.FastqKMerMatcher(k31.store)
    m.set_taxids(sdb.taxids)
    lib = ga.lib()
    import ctypes as C
    ptrs, want = [], []
    for j, (a, b) in enumerate(((0, 100), (100, 250), (250, 300))):
        _submit(m, _text(recs[a:b]))
        p, nb, nl = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        assert lib.gs_match_kraken_text(m.h, 1, j & 1, C.byref(p), C.byref(nb), C.byref(nl)) == 0
        ptrs.append((p.value, nb.value))
        want.append(b"".join(lines[a:b]))
        assert nb.value == len(want[-1]) and nl.value == b - a
        if j == 1:  # the text of slot 0 after the slot-1 call
            assert ga.binding._fetch_device(0, C.c_void_p(ptrs[0][0]), ptrs[0][1]).tobytes() == want[0]
    assert ga.binding._fetch_device(0, C.c_void_p(ptrs[1][0]), ptrs[1][1]).tobytes() == want[1]
    assert ga.binding._fetch_device(0, C.c_void_p(ptrs[2][0]), ptrs[2][1]).tobytes() == want[2]
    m.close()


def test_state_errors(sdb, k31, cycle):
    import ctypes as C
    recs, cv, lines = cycle
    lib = ga.lib()
    text = _text(recs[:20])

    def call(m, slot=0, args=None):
        p, nb, nl = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        a = args or (C.byref(p), C.byref(nb), C.byref(nl))
        return lib.gs_match_kraken_text(m.h, 1, slot, *a)

    m = ga.FastqKMerMatcher(k31.store)
    m.set_taxids(sdb.taxids)
    assert call(m) == GS_E_STATE  # no chunk has been submitted
    _submit(m, text)
    assert call(m, 2) == GS_E_INVALID and call(m, -1) == GS_E_INVALID
    assert call(m, 0, (None, None, None)) == GS_E_INVALID
    assert call(m) == 0
    m.submit_text(np.frombuffer(text, dtype=np.uint8))  # without a class array
    assert call(m) == GS_E_STATE
    m.submit_fasta(np.frombuffer(b">a\n" + recs[0][1] + b"\n", dtype=np.uint8))
    assert call(m) == GS_E_STATE  # FASTA
    _submit(m, text)
    assert call(m) == 0
    ml = b"@a\n" + recs[0][1][:75] + b"\n" + recs[0][1][75:] + b"\n+\n" + b"I" * 150 + b"\n"
    m.submit_fastq_ml(np.frombuffer(ml, dtype=np.uint8))
    assert call(m) == GS_E_STATE  # general FASTQ
    m.close()

    m = ga.FastqKMerMatcher(k31.store)
    _submit(m, text)
    assert call(m) == GS_E_STATE  # no taxids
    assert lib.gs_match_set_taxids(m.h, (C.c_char_p * sdb.n_values)()) == GS_E_INVALID  # NULL entries
    assert call(m) == GS_E_STATE
    m.set_taxids(sdb.taxids)
    assert call(m) == 0
    _submit(m, b"@a\nACGT\n+\nIIII\n@b\nACGT\n-\nIIII\n")  # refused by the record scan: no '+' line
    assert call(m) == GS_E_STATE
    m.text_clear_error()
    _submit(m, text)
    assert call(m) == 0
    m.close()
