"""gs_*_compact_records and gs_match_kraken_records: the per-read outputs of FASTA and general FASTQ chunks written on the device,
byte for byte against ReadEntry.write over streamgoals.read_entries and against the plain-Python rule of tests/krakenlines.py over
the oracle's classes and segments -- at every record shape, selection, seam of the block scan, boundary of the 16-byte words and the
4096-byte pieces, both slots and every state error.  Needs an MI355X: run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import genestrip_amd as ga
import recordtext as rt
from genestrip_amd import synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

GS_E_INVALID, GS_E_STATE, GS_E_UNSUPPORTED = -1, -5, -4
TREE3 = np.array([-1, 0, 0], dtype=np.int32)
TAX3 = ["", "5", "1234567"]


@pytest.fixture(scope="module")
def sdb():
    return synth.SynthDB(genera=3, species_per_genus=3, genome_len=20000, seed=11)


@pytest.fixture(scope="module")
def k31(sdb):
    s = rt.Side(ga, 31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    yield s
    s.close()


@pytest.fixture(scope="module")
def k2():
    d = {}
    for s, vi in (("CC", 0), ("TT", 1), ("AG", 2)):
        d.setdefault(orc.kmer_canonical(s), vi)
    keys = sorted(d)
    s = rt.Side(ga, 2, np.array(keys, dtype=np.int64), np.array([d[x] for x in keys], dtype=np.int32), 3, TREE3)
    yield s
    s.close()


@pytest.fixture(scope="module")
def blooms(sdb):
    """a filter on the device that holds the k-mers of some species, and the same filter in the oracle"""
    keys = sdb.kmers[np.isin(sdb.value_idx, sdb.species_vi)]
    ob = orc.Bloom(orc.BLOOM_XOR, len(keys), 1e-8)
    ob.put_many(keys)
    return ga.DeviceBloomFilter(ga.BLOOM_XOR, ob.bits, ob.hash_factors, ob.words), ob


@pytest.fixture(scope="module")
def reads(sdb):
    """300 reads of 150 bases, every third one random (hits neither the store nor the filter)"""
    seq, off = synth.reads_host(sdb.genomes, 300, seed=9)
    rng = np.random.default_rng(1)
    out = []
    for i in range(300):
        r = bytes(seq[int(off[i]):int(off[i + 1])])
        if i % 3 == 0:
            r = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 150))
        out.append(r)
    return out


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _qual(rng, n):
    return bytes(b"IJKL#~5"[x] for x in rng.integers(0, 7, n))


def _bases(rng, n):
    return bytes(b"ACGT"[x] for x in rng.integers(0, 4, n))


def _same(got, want, what):
    got, want = bytes(got), bytes(want)
    if got != want:
        i = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}, first difference at {i}: {got[max(0, i - 30):i + 30]!r} / {want[max(0, i - 30):i + 30]!r}")


def _reads_chunk(rd, text, key, is_fasta, both_probs=(True, False), slot=0):
    """one chunk through a gs_reads handle and through the rule; -> (entries, keep flags)"""
    if is_fasta:
        used, acc = len(text), rd.select_fasta(text, key)
    else:
        n_rec, used, acc = rd.select_fastq_ml(text, key)
        assert n_rec >= 0
    ents = rt.entries(text[:used], is_fasta)
    keep = [d[1:1 + len(key)] == key for d, _, _ in ents]
    assert len(acc) == len(ents) and acc.astype(bool).tolist() == keep
    for probs in both_probs:
        got, n = rd.compact_records(probs, slot)
        _same(got, rt.record_text(ents, keep, probs), f"probs {probs}")
        assert n == sum(keep)
    return ents, keep


@pytest.mark.parametrize("crlf", [False, True])
def test_fastq_record_shapes(crlf):
    """1 .. 3 sequence lines, qualities over another number of lines, a last quality line that overshoots, descriptor lengths 2 .. 17,
    half a record at the end; with and without qualities"""
    rng = np.random.default_rng(5)
    recs, i = [], 0
    for n_seq in (1, 2, 3):
        for n_qual in (1, 2, 3):
            for over in (2, 3, 20) if crlf else (0, 1, 20):
                for L in (7, 40, 151):
                    d = (b"@K" if i % 3 else b"@Z") + b"d" * (i % 16)  # 2 .. 17 bytes: record boundaries at every offset mod 16
                    recs.append((d, _bases(rng, L), _qual(rng, L + over), n_seq, n_qual))
                    i += 1
    text = rt.fastq_ml(recs, crlf)
    half = rt.fastq_ml([(b"@Khalf", _bases(rng, 90), _qual(rng, 93), 3, 1)], crlf)
    half = half[:half.index(b"+")]  # the record's sequence lines, no '+' line yet
    rd = ga.DeviceReads()
    ents, keep = _reads_chunk(rd, text + half, b"K", False)
    assert len(ents) == len(recs) and 0 < sum(keep) < len(keep)
    assert any(len(q) > len(r) for _, r, q in ents) and [e[1] for e in ents[:3]] == [rt.entries(text, False)[j][1] for j in range(3)]
    if crlf:
        assert all(d.endswith(b"\r") and r.endswith(b"\r") and q.endswith(b"\r") for d, r, q in ents)
    rd.close()


def test_odd_descriptors_through_the_filter(blooms, reads):
    """a descriptor of one byte, one that does not start with '@', an empty descriptor line if the record search takes it: only a
    filter (or a match) writes such a record -- no key selects it.  The two outputs partition the chunk."""
    bloom, ob = blooms
    rng = np.random.default_rng(2)
    descs = [b"@", b"Xno-at", b"@a b", b"@", b"@last"]
    recs = [(d, reads[i], _qual(rng, 150 + (i % 2) * 7), 1 + i % 3, 1 + (i + 1) % 3) for i, d in enumerate(descs)]
    f = ga.FastqBloomFilter(31, bloom)
    for with_empty in (True, False):
        rr = recs[:2] + [(b"", reads[7], _qual(rng, 150), 2, 2)] + recs[2:] if with_empty else recs
        text = rt.fastq_ml(rr)
        acc = np.zeros(len(text) // 4 + 2, dtype=np.uint8)
        n_rec, used, _ = f.submit_fastq_ml(text, acc)
        if n_rec < 0:  # the record search refuses an empty descriptor line: the host parser's case, nothing to write here
            assert with_empty
            f.text_reset()
            continue
        assert n_rec == len(rr) and used == len(text)
        ents = rt.entries(text, False)
        seq, off = orc.pack_reads([r for _, r, _ in ents])
        want = ob.filter_batch(31, 1, 0.2, seq, off).astype(bool)
        for probs in (True, False):
            a, na = f.compact_records(1, probs, 0)
            r, nr = f.compact_records(0, probs, 0)
            assert acc[:n_rec].astype(bool).tolist() == want.tolist() and 0 < want.sum() < n_rec
            _same(a, rt.record_text(ents, want, probs), "accepted")
            _same(r, rt.record_text(ents, ~want, probs), "rest")
            assert na + nr == n_rec and len(a) + len(r) == len(rt.record_text(ents, [True] * n_rec, probs))


def _fasta_chunk(reads, rng, crlf=False):
    """header-only records at the start, in the middle and at the end; header lengths 1 .. 17"""
    recs = [(b">Kempty0", b"")]
    for i in range(1, 18):
        recs.append(((b">K" + b"h" * 15)[:i] if i % 2 else (b">Z some text here")[:i], reads[i] if i % 4 else reads[i][:61]))
        if i == 9:
            recs.append((b">Kempty1 x", b""))
    recs.append((b">Kempty2", b""))
    return rt.fasta(recs, 60, crlf), recs


@pytest.mark.parametrize("crlf", [False, True])
def test_fasta_through_match_filter_and_reads(k31, blooms, reads, crlf):
    rng = np.random.default_rng(8)
    text, recs = _fasta_chunk(reads, rng, crlf)
    ents = rt.entries(text, True)
    n = len(ents)
    assert n == len(recs) and ents[0][1] == b"" and ents[-1][1] == b"" and ents[0][0] == b"@Kempty0" + (b"\r" if crlf else b"")
    # match: the reads matchRead returned
    cv_want, fl_want = k31.match([r for _, r, _ in ents])
    keep = (fl_want & orc.F_RETURNED) != 0
    assert 0 < keep.sum() < n
    m = ga.FastqKMerMatcher(k31.store)
    cv, fl = np.full(n, -7, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    m.submit_fasta(_u8(text), class_vi=cv, flags=fl)
    for probs, slot in ((False, 0), (True, 1)):
        got, nr = m.compact_records(probs, slot)
        _same(got, rt.record_text(ents, keep, False), "match")
        assert nr == keep.sum()
    assert np.array_equal(fl, fl_want) and np.array_equal(cv, cv_want)
    m.close()
    # filter: accepted and rest partition the chunk
    bloom, ob = blooms
    seq, off = orc.pack_reads([r if r else b"" for _, r, _ in ents])
    want = ob.filter_batch(31, 1, 0.2, seq, off).astype(bool)
    f = ga.FastqBloomFilter(31, bloom)
    acc = np.zeros(n, dtype=np.uint8)
    f.submit_fasta(text, acc)
    lib = ga.lib()
    pa, pr, nb_a, nb_r, cnt = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert lib.gs_filter_compact_records(bloom.h, 1, 1, 1, C.byref(pa), C.byref(nb_a), C.byref(cnt)) == 0
    na = cnt.value
    assert lib.gs_filter_compact_records(bloom.h, 0, 1, 1, C.byref(pr), C.byref(nb_r), C.byref(cnt)) == 0
    nr = cnt.value
    # the two files of a chunk are written side by side: the accepted text is still there after the rest has been made in the same slot
    a, r = ga.binding._fetch_device(0, pa, nb_a.value), ga.binding._fetch_device(0, pr, nb_r.value)
    assert acc.astype(bool).tolist() == want.tolist() and 0 < want.sum() < n
    _same(a, rt.record_text(ents, want, False), "accepted")
    _same(r, rt.record_text(ents, ~want, False), "rest")
    assert na + nr == n
    # reads: by key; a header-only record is "@h\n\n+\n\n"
    rd = ga.DeviceReads()
    _reads_chunk(rd, text, b"K", True)
    got, _ = rd.compact_records(True, 0)
    assert bytes(got).startswith(ents[0][0] + b"\n\n+\n\n") and bytes(got).endswith(ents[-1][0] + b"\n\n+\n\n")
    rd.close()


@pytest.mark.parametrize("which", ["none", "all", "first", "last"])
def test_selections(reads, which):
    n = 40
    sel = {"none": [], "all": list(range(n)), "first": [0], "last": [n - 1]}[which]
    rng = np.random.default_rng(3)
    desc = lambda i: (b"@K%d" if i in sel else b"@Z%d") % i
    rd = ga.DeviceReads()
    fa = rt.fasta([(b">" + desc(i)[1:], reads[i][:100 + i]) for i in range(n)], 70)
    ents, keep = _reads_chunk(rd, fa, b"K", True)
    assert [i for i, k in enumerate(keep) if k] == sel
    fq = rt.fastq_ml([(desc(i), reads[i][:100 + i], _qual(rng, 100 + i + i % 3), 1 + i % 3, 1 + i % 2) for i in range(n)])
    ents, keep = _reads_chunk(rd, fq, b"K", False)
    assert [i for i, k in enumerate(keep) if k] == sel
    rd.close()


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_record_counts_across_the_block_scan(reads, n):
    rng = np.random.default_rng(n)
    rd = ga.DeviceReads()
    fa = rt.fasta([((b">K%d" if i % 5 else b">Z%d") % i, b"" if i % 11 == 5 else reads[i % 300][:20 + i % 90]) for i in range(n)], 50)
    ents, _ = _reads_chunk(rd, fa, b"K", True)
    assert len(ents) == n
    fq = rt.fastq_ml([((b"@K%d" if i % 7 else b"@Z%d") % i, reads[i % 300][:20 + i % 90], _qual(rng, 20 + i % 90 + (9 if i % 5 == 0 else 0)), 1 + i % 3, 1 + (i // 3) % 3)
                      for i in range(n)])
    ents, _ = _reads_chunk(rd, fq, b"K", False)
    assert len(ents) == n
    rd.close()


@pytest.mark.parametrize("total", [4095, 4096, 4097, 8191, 8192, 8193])
def test_totals_around_the_pieces(reads, total):
    """two records whose text ends just below, at or just above one and two pieces of the copy"""
    first = (b">K1", reads[1][:100])  # 3 + 2 * 100 + 5 bytes of text
    rest = total - 208
    hl = 3 if rest % 2 == 0 else 4
    L = (rest - hl - 5) // 2
    long = b"".join(reads[:40])[:L]
    fa = rt.fasta([first, ((b">K2x")[:hl], long)], 80)
    rd = ga.DeviceReads()
    ents, keep = _reads_chunk(rd, fa, b"K", True)
    assert len(rt.record_text(ents, keep, False)) == total
    rd.close()


def test_a_record_of_more_than_two_pieces(reads):
    rng = np.random.default_rng(6)
    long = b"".join(reads[:60])  # 9000 bases: 18 000 bytes of text and more
    rd = ga.DeviceReads()
    fq = rt.fastq_ml([(b"@Kshort", reads[0], _qual(rng, 150), 1, 1), (b"@Klong one", long, _qual(rng, len(long) + 5), 3, 2), (b"@Kend", reads[1], _qual(rng, 151), 2, 2)])
    ents, keep = _reads_chunk(rd, fq, b"K", False)
    assert len(rt.record_text(ents[1:2], [True], True)) > 2 * 4096 + 16
    fa = rt.fasta([(b">Kshort", reads[0]), (b">Klong one", long), (b">Kend", reads[1])], 60)
    _reads_chunk(rd, fa, b"K", True)
    rd.close()


def test_slots_keep_their_text(reads):
    lib = ga.lib()
    rd = ga.DeviceReads()
    rng = np.random.default_rng(9)
    ptrs, want = [], []
    for j, (a, b) in enumerate(((0, 30), (30, 80), (80, 100))):
        fq = rt.fastq_ml([(b"@K%d" % i, reads[i], _qual(rng, 150 + i % 4), 1 + i % 2, 1 + i % 3) for i in range(a, b)])
        rd.select_fastq_ml(fq, b"K")
        p, nb, nr = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        assert lib.gs_reads_compact_records(rd.h, 1, j & 1, C.byref(p), C.byref(nb), C.byref(nr)) == 0
        ptrs.append((p.value, nb.value))
        want.append(rt.record_text(rt.entries(fq, False), [True] * (b - a), True))
        assert nb.value == len(want[-1]) and nr.value == b - a
        if j == 1:  # the text of slot 0 after the slot-1 call
            assert ga.binding._fetch_device(0, C.c_void_p(ptrs[0][0]), ptrs[0][1]).tobytes() == want[0]
    assert ga.binding._fetch_device(0, C.c_void_p(ptrs[1][0]), ptrs[1][1]).tobytes() == want[1]
    assert ga.binding._fetch_device(0, C.c_void_p(ptrs[2][0]), ptrs[2][1]).tobytes() == want[2]
    rd.close()


def _kraken_chunk(side, m, text, is_fasta, taxids, segments_too=False, **cfg):
    n_max = text.count(b"\n") // (1 if is_fasta else 4) + 2
    cv, fl = np.full(n_max, -7, dtype=np.int32), np.zeros(n_max, dtype=np.uint8)
    if is_fasta:
        m.submit_fasta(_u8(text), class_vi=cv, flags=fl)
        used = len(text)
    else:
        _, used = m.submit_fastq_ml(_u8(text), class_vi=cv, flags=fl)
    ents = rt.entries(text[:used], is_fasta)
    cv_want, _ = side.match([r for _, r, _ in ents], **cfg)
    out = {}
    for write_all, slot in ((True, 0), (False, 1)):
        got = m.kraken_records(write_all, slot)
        want = rt.kraken_text(ents, side.k, side.segments, cv_want, taxids, write_all)
        glines, wlines = got.split(b"\n"), want.split(b"\n")
        for i, (a, b) in enumerate(zip(glines, wlines)):
            assert a == b, f"line {i}: device {a[:200]!r} rule {b[:200]!r}"
        assert got == want and m.kraken_lines == want.count(b"\n")
        out[write_all] = got
    assert np.array_equal(cv[:len(ents)], cv_want)
    if segments_too:  # the call has left this chunk's segments where gs_match_segments_fetch finds them
        per_read = [side.segments(r) if len(r) >= side.k else [] for _, r, _ in ents]
        codes, starts = m.segments_fetch(sum(len(p) for p in per_read))
        at = 0
        for (_, r, _), p in zip(ents, per_read):
            st = starts[at:at + len(p)].tolist()
            cnt = [b - a for a, b in zip(st, st[1:] + [len(r) - side.k + 1])]
            assert list(zip(codes[at:at + len(p)].tolist(), cnt)) == p
            at += len(p)
    return ents, cv_want, out


def test_kraken_lines_of_record_chunks(sdb, k31, reads):
    rng = np.random.default_rng(12)
    names = [b"noblank", b"cut here", b"n" * 300 + b" tail", b"", b"a\tb x", b"q" * 5000]
    g = sdb.genomes
    long = bytes(g[3]) + bytes(g[4, :13000])  # 33 000 bases: the segments come in pieces, the line goes the block's way
    assert len(long) == 33000
    m = ga.FastqKMerMatcher(k31.store)
    m.set_taxids(sdb.taxids)
    fa = [(b">" + nm, reads[i] if i != 3 else reads[0]) for i, nm in enumerate(names)]
    fa += [(b">empty in the middle", b""), (b">long", long), (b">tail", reads[9][:30]), (b">lastempty", b"")]
    ents, cv, out = _kraken_chunk(k31, m, rt.fasta(fa, 60), True, sdb.taxids, segments_too=True)
    assert b"\t33000\t" in out[True] and b"\tnoblank\t" in out[True] and b"\tcut\t" in out[True] and b"q" * 5000 in out[True]
    assert out[True].count(b"\n") == len(fa) - 3  # (no line: the two records without a sequence, the one shorter than k)
    assert (cv < 0).any() and 0 < out[False].count(b"\n") < out[True].count(b"\n") and b"U\t" in out[True]
    fq = [(b"@" + nm, reads[i], _qual(rng, 150 + i), 1 + i % 3, 1 + (i + 1) % 3) for i, nm in enumerate(names)]
    half = b"@half\nACGT\nAC\n"
    ents, cv, out = _kraken_chunk(k31, m, rt.fastq_ml(fq) + half, False, sdb.taxids, segments_too=True)
    assert len(ents) == len(fq) and out[True].count(b"\n") == len(fq)
    crlf = rt.fastq_ml([(b"@name", reads[1], _qual(rng, 154), 2, 1)], True)
    _, _, out = _kraken_chunk(k31, m, crlf, False, sdb.taxids)
    assert b"\tname\r\t" in out[True] and b"\t152\t" in out[True]  # the '\r's of the descriptor and of both sequence lines are kept and counted
    m.close()


def test_kraken_reads_of_many_segments_at_small_k(k2):
    rng = np.random.default_rng(4)
    rs = [_bases(rng, int(rng.integers(3, 401))) for _ in range(300)]
    assert max(len(k2.segments(r)) for r in rs) > 32 and min(len(k2.segments(r)) for r in rs) <= 32  # (before the device is touched)
    m = ga.FastqKMerMatcher(k2.store, ga.MatchConfig(max_paths=4))
    m.set_taxids(TAX3)
    _kraken_chunk(k2, m, rt.fasta([(b">r%d x" % i, r) for i, r in enumerate(rs)], 70), True, TAX3, segments_too=True, max_paths=4)
    fq = rt.fastq_ml([(b"@r%d x" % i, r, _qual(rng, len(r) + i % 2), 1 + i % 3, 1 + i % 2) for i, r in enumerate(rs)])
    _kraken_chunk(k2, m, fq, False, TAX3, max_paths=4)
    m.close()


def test_state_errors(sdb, k31, blooms, reads):
    lib = ga.lib()
    rng = np.random.default_rng(1)
    fa = rt.fasta([(b">K%d" % i, reads[i]) for i in range(5)])
    fq = rt.fastq_ml([(b"@K%d" % i, reads[i], _qual(rng, 150), 2, 1) for i in range(5)])
    four = b"".join(b"@K%d\n" % i + reads[i] + b"\n+\n" + b"I" * 150 + b"\n" for i in range(5))

    def out():
        return [C.byref(x) for x in (C.c_void_p(), C.c_int64(0), C.c_int64(0))]

    # reads
    rd = ga.DeviceReads()
    call = lambda slot=0, a=None: lib.gs_reads_compact_records(rd.h, 1, slot, *(a or out()))
    assert call() == GS_E_STATE  # no chunk
    rd.select_text(four, b"K")
    assert call() == GS_E_STATE  # four-line
    rd.select_fasta(fa, b"K")
    assert call(2) == GS_E_INVALID and call(-1) == GS_E_INVALID and call(0, (None, None, None)) == GS_E_INVALID
    assert call() == 0
    rd.fasta2fastq(fa)
    assert call() == GS_E_STATE  # a chunk without per-read flags
    rd.select_fastq_ml(fq, b"K")
    assert call() == 0
    assert lib.gs_reads_compact_text(rd.h, 1, 0, *out()) == GS_E_UNSUPPORTED  # the old call keeps its answer
    p, nb, nr = C.c_void_p(), C.c_int64(7), C.c_int64(7)
    rd.select_fasta(b"", b"K")
    assert lib.gs_reads_compact_records(rd.h, 1, 0, C.byref(p), C.byref(nb), C.byref(nr)) == 0 and nb.value == 0 and nr.value == 0
    rd.select_fasta(b">a\n\nAC\n", b"K")  # an empty line: refused by the FASTA record search
    assert rd.text_status()[0] >= 0 and call() == GS_E_STATE
    rd.close()

    # filter
    _, ob = blooms
    bloom = ga.DeviceBloomFilter(ga.BLOOM_XOR, ob.bits, ob.hash_factors, ob.words)  # (a handle no chunk has gone through)
    f = ga.FastqBloomFilter(31, bloom)
    call = lambda which=1: lib.gs_filter_compact_records(bloom.h, which, 1, 0, *out())
    assert call() == GS_E_STATE
    acc = np.zeros(16, dtype=np.uint8)
    f.submit_text(four, acc)
    assert call() == GS_E_STATE
    f.submit_fasta(fa, acc)
    assert call() == 0 and call(0) == 0
    assert lib.gs_filter_compact_text(bloom.h, 1, 1, 0, *out()) == GS_E_STATE  # needs a four-line chunk
    f.submit_fastq_ml(fq, acc)
    assert call() == 0
    f.sync()

    # match
    m = ga.FastqKMerMatcher(k31.store)
    rec = lambda: lib.gs_match_compact_records(m.h, 1, 0, *out())
    kr = lambda: lib.gs_match_kraken_records(m.h, 1, 0, *out())
    assert rec() == GS_E_STATE and kr() == GS_E_STATE
    cv, fl = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.uint8)
    m.submit_fasta(_u8(fa), class_vi=cv, flags=fl)
    assert rec() == 0 and kr() == GS_E_STATE  # no taxids
    m.set_taxids(sdb.taxids)
    assert kr() == 0
    assert lib.gs_match_kraken_text(m.h, 1, 0, *out()) == GS_E_STATE and lib.gs_match_compact_text(m.h, 1, 0, *out()) == GS_E_STATE
    m.submit_fasta(_u8(fa))  # without flags and classes
    assert rec() == GS_E_STATE and kr() == GS_E_STATE
    m.submit_fastq_ml(_u8(fq), class_vi=cv, flags=fl)
    assert rec() == 0 and kr() == 0
    assert lib.gs_match_kraken_text(m.h, 1, 0, *out()) == GS_E_STATE
    m.submit_text(_u8(four), class_vi=cv, flags=fl)
    assert rec() == GS_E_STATE and kr() == GS_E_STATE  # four-line
    m.submit_fasta(_u8(b">a\n\nAC\n"), class_vi=cv, flags=fl)
    assert m.text_status()[0] >= 0
    assert rec() == GS_E_STATE and kr() == GS_E_STATE  # refused
    m.text_clear_error()
    m.submit_fasta(_u8(fa), class_vi=cv, flags=fl)
    assert rec() == 0 and kr() == 0
    m.close()
