"""host.genome_files (gs_host_genome_files: genome FASTA files -> regions on the device -> the _add calls of the region stage)
against the plain restatement of the reference's walk (tests/genomefasta.py) fed to the same handles from host memory: the dengue
fixture, a collection of mixed line shapes as a plain file, gzip and BGZF at reader blocks that put the cuts everywhere, all four
region handles, a chunk the device refuses, and a callback's error code.  Needs an MI355X: run with -m gpu."""
import gzip
import os

import numpy as np
import pytest

import genestrip_amd as ga
import genomefasta as gf
from conftest import GOLDEN, bgzf
from genestrip_amd import host
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

PARENT = np.array([-1, 0, 1, 1, 2, 4, 0], dtype=np.int32)  # T/tax/TaxTreeLCATest.java:51
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
K = 31


def _rule(header):
    """this test's resolver: `>r<i> ...` counts for node i % 7 if i is even, else it is skipped"""
    i = int(header[2:].split()[0])
    return i % 7 if i % 2 == 0 else -1


def _resolve(_file, _first, headers):
    return [_rule(h) for h in headers]


def _reference_regions(data):
    """the restatement's regions under the same rule, in host memory: (seq, offsets, vi)"""
    headers, seq, offsets, _, _ = gf.read_fasta(data, True)
    vi = [_rule(h) for h in headers]
    parts = [seq[offsets[i]:offsets[i + 1]] for i in range(len(headers)) if vi[i] >= 0]
    flat = np.frombuffer(b"".join(parts) or b"\x00", dtype=np.uint8)
    return flat, np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64), np.array([v for v in vi if v >= 0], np.int32)


def _collection(seed=21, n=40):
    """about 40 records: wrapped at several widths, unwrapped, CRLF, empty, with empty lines, lower case and N; sizes up to 9 kB"""
    rng = np.random.default_rng(seed)
    core = ACGT[rng.integers(0, 4, 4000)].tobytes()  # shared between records: the update walk has something to fold
    recs = []
    for i in range(n):
        eol = b"\r\n" if i % 4 == 1 else b"\n"
        size = 0 if i % 9 == 4 else int(rng.integers(40, 9000))
        body = bytearray(core[:size // 2] + ACGT[rng.integers(0, 4, size - size // 2)].tobytes())
        if size > 100:
            body[50:53] = b"acn"
            body[70] = ord("N")
        w = [60, 70, 80, 1 << 20, 61, 17][i % 6]
        lines = [bytes(body[j:j + w]) for j in range(0, size, w)]
        if i % 5 == 3 and lines:
            lines.insert(len(lines) // 2, b"")
        recs.append(b">r%d genome %d" % (i, i) + eol + b"".join(x + eol for x in lines))
    return b"some text in front of the first header\n" + b"".join(recs)


def _build(feed):
    """fill walk, update walk, finish -> (kmers, value_idx); feed(add) walks the collection once into add(seq, off, vi)"""
    b = ga.DeviceDbBuilder(K, len(PARENT), PARENT)
    feed(lambda s, o, v: b.add(s, o, v, update=False))
    feed(lambda s, o, v: b.add(s, o, v, update=True))
    out = b.finish()
    b.close()
    return out


@pytest.fixture(scope="module")
def collection():
    data = _collection()
    regions = _reference_regions(data)
    assert len(regions[2]) == 20 and 60_000 < len(regions[0])
    want = _build(lambda add: add(*regions))
    assert len(want[0]) > 50_000 and len(set(want[1].tolist())) > 3
    return data, regions, want


def test_dengue_fixture_through_the_file_loop():
    path = os.path.join(GOLDEN, "dengue1", "dengue1.fasta")
    parent = np.array([-1], np.int32)
    b = ga.DeviceDbBuilder(K, 1, parent)
    t = host.genome_files([path], lambda f, first, headers: [0] * len(headers), lambda s, o, v: b.add(s, o, v))
    got = b.finish()
    b.close()
    assert len(got[0]) == 10705
    assert t.records == t.kept_records == 1 and t.host_chunks == 0 and t.chunks >= 1
    raw = open(path, "rb").read()
    headers, seq, offsets, _, _ = gf.read_fasta(raw)
    assert t.kept_bases == len(seq) and len(headers) == 1
    flat, off = np.frombuffer(seq, np.uint8), np.array(offsets, np.uint64)
    b = ga.DeviceDbBuilder(K, 1, parent)
    b.add(flat, off, np.zeros(1, np.int32))
    want = b.finish()
    b.close()
    ob = orc.DbBuild(K, 1, parent, True, 1, -1)
    ob.fill(flat, off, np.zeros(1, np.int32))
    ob.optimize()
    ref = ob.fetch()
    ob.close()
    for x in (want, ref):
        assert np.array_equal(got[0], x[0]) and np.array_equal(got[1], x[1])


@pytest.mark.parametrize("form,block", [("plain", 64), ("plain", 1000), ("plain", 4096), ("plain", 65536), ("plain", 1 << 22),
                                        ("gz", 65536), ("gz", 1 << 22), ("bgzf", 65536), ("bgzf", 1 << 22)])
def test_collection_as_plain_gzip_and_bgzf_at_many_block_sizes(collection, tmp_path, monkeypatch, form, block):
    data, regions, want = collection
    path = tmp_path / ("genomes.fasta" + ("" if form == "plain" else ".gz"))
    path.write_bytes(data if form == "plain" else gzip.compress(data, 6) if form == "gz" else bgzf(data))
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", str(block))
    totals = []
    got = _build(lambda add: totals.append(host.genome_files([path], _resolve, add)))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for t in totals:
        assert (t.records, t.kept_records, t.kept_bases) == (40, 20, int(regions[1][-1]))
        assert t.max_line_bytes == max(len(x) + 1 for x in data.split(b"\n"))
    if form == "plain" or block >= 65536:  # (a plain file whose records outgrow a block goes on with larger blocks, on the device)
        assert totals[0].host_chunks == 0
    if form == "plain" and block == 65536:
        assert totals[0].chunks >= 3


def test_two_files_and_first_record(collection, tmp_path):
    data, regions, want = collection
    at = data.index(b">r17 ")
    a, b = tmp_path / "a.fasta", tmp_path / "b.fasta.gz"
    a.write_bytes(data[:at])
    b.write_bytes(gzip.compress(data[at:]))
    seen = []

    def resolve(file, first, headers):
        seen.append((file, first, len(headers)))
        return _resolve(file, first, headers)

    got = _build(lambda add: host.genome_files([a, b], resolve, add))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for f, n in ((0, 17), (1, 23)):
        mine = [(first, m) for file, first, m in seen[:len(seen) // 2] if file == f]
        assert mine[0][0] == 0 and sum(m for _, m in mine) == n
        assert all(mine[i + 1][0] == mine[i][0] + mine[i][1] for i in range(len(mine) - 1))


def test_sizer_updater_and_quality_take_the_same_regions(collection, tmp_path):
    data, regions, want = collection
    path = tmp_path / "genomes.fasta"
    path.write_bytes(data)
    walk = lambda add: host.genome_files([path], _resolve, add)
    direct = lambda add: add(*regions)

    def sizer(feed):
        s = ga.DeviceDbSizer(K, len(PARENT))
        feed(s.add)
        t, per_value, hist = s.counts()
        s.close()
        return (t.total, t.dust, t.included), per_value, hist

    a, b = sizer(walk), sizer(direct)
    assert a[0] == b[0] and a[0][0] > 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])

    fb = ga.DeviceDbBuilder(K, len(PARENT), PARENT)
    fb.add(*regions)
    filled = fb.finish()
    fb.close()

    def updater(feed):
        u = ga.DeviceDbUpdater.from_arrays(K, filled[0], filled[1], len(PARENT), PARENT)
        feed(u.add)
        moved = u.finish()
        out = u.fetch()
        u.close()
        return moved, out

    a, b = updater(walk), updater(direct)
    assert a[0] == b[0] and np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1]) and len(a[1][0]) == len(filled[0])

    store = ga.DeviceKMerStore(K, want[0], want[1], len(PARENT), PARENT)

    def quality(feed):
        q = ga.DeviceDbQuality(store)
        feed(q.add)
        out = q.finish()
        q.close()
        return out

    a, b = quality(walk), quality(direct)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0][:, 0].sum() > 0
    store.close()


@pytest.mark.parametrize("form", ["plain", "gz", "bgzf"])
def test_record_longer_than_a_block(tmp_path, monkeypatch, form):
    """records of 300 kB and 150 kB between small ones at blocks of 64 KiB: the file goes on from the long record with blocks twice
    as large and stays on the device -- a plain file is read from there, a gzip stream is inflated from its start again and what an
    earlier pass has worked off is passed over: every record reaches the resolver once, in order"""
    rng = np.random.default_rng(31)
    body = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()
    recs = [b">r%d small\n" % i + body(3000) + b"\n" for i in range(30)]
    recs[12] = b">r12 long\n" + b"".join(body(70) + b"\n" for _ in range(4300))
    recs[20] = b">r20 long and unwrapped\n" + body(150_000) + b"\n"
    data = b"".join(recs)
    want = _build(lambda add: add(*_reference_regions(data)))
    path = tmp_path / ("long.fasta" + ("" if form == "plain" else ".gz"))
    path.write_bytes(data if form == "plain" else gzip.compress(data) if form == "gz" else bgzf(data))
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    totals, seen = [], []

    def resolve(file, first, headers):
        seen.append((first, [int(h[2:].split()[0]) for h in headers]))
        return _resolve(file, first, headers)

    got = _build(lambda add: totals.append(host.genome_files([path], resolve, add)))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert totals[0].records == 30 and totals[0].kept_records == 15
    first_walk = seen[:len(seen) // 2]
    assert [i for _, ids in first_walk for i in ids] == list(range(30)) and all(f == ids[0] for f, ids in first_walk)
    # on the device throughout: the 36 kB of records in front of the first long one in the first pass, the rest in a later one
    assert totals[0].host_chunks == 0 and totals[0].chunks >= 2


def test_chunk_with_a_nul_byte_takes_the_host_parser(collection, tmp_path, monkeypatch):
    data, _, _ = collection
    at = data.index(b">r20 ") + 200
    bad = data[:at] + b"\x00" + data[at:]
    want = _build(lambda add: add(*_reference_regions(bad)))
    path = tmp_path / "nul.fasta"
    path.write_bytes(bad)
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "16384")
    totals = []
    got = _build(lambda add: totals.append(host.genome_files([path], _resolve, add)))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert totals[0].host_chunks == 1 and totals[0].chunks > 5 and totals[0].records == 40


def test_everything_through_the_host_parser_gives_the_same(collection, tmp_path, monkeypatch):
    data, _, want = collection
    path = tmp_path / "genomes.fasta.gz"
    path.write_bytes(gzip.compress(data))
    monkeypatch.setenv("GS_HOST_FAST", "0")
    totals = []
    got = _build(lambda add: totals.append(host.genome_files([path], _resolve, add)))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert totals[0].host_chunks == totals[0].chunks >= 1


def test_a_callback_ends_the_walk_with_its_code(collection, tmp_path):
    data, _, _ = collection
    path = tmp_path / "genomes.fasta"
    path.write_bytes(data)
    calls = []
    with pytest.raises(ga.GsError) as e:
        host.genome_files([path, path], lambda f, first, headers: 77, lambda s, o, v: calls.append(1))
    assert e.value.code == 77 and not calls
    with pytest.raises(ga.GsError) as e:
        host.genome_files([path], _resolve, lambda s, o, v: 31)
    assert e.value.code == 31
    with pytest.raises(KeyError):
        host.genome_files([path], lambda f, first, headers: {}["no such accession"], lambda s, o, v: None)
    with pytest.raises(ga.GsError) as e:
        host.genome_files([tmp_path / "missing.fasta"], _resolve, lambda s, o, v: None)
    assert e.value.code in (-1, -7)
