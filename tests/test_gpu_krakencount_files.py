"""host.kraken_count_files on the device path against the plain-Python restatement of the reference (tests/krakencount.py): every
container format at block sizes that cut chunks inside lines, refused regions that the line-by-line parser takes over, several
files, the tax id selection, the CSV, failures -- and the round trip: a match run writes its Kraken-style lines on the device, the
file is counted on the device, and the counts must add up to the run's own table.  Needs an MI355X: run with -m gpu."""
import gzip
import os
import re

import numpy as np
import pytest

import genestrip_amd as ga
import krakencount as kc
from conftest import bgzf
from genestrip_amd import host, synth
from krakencount_cases import LONG_LINE, check_identities, line, long_line, random_text, sample_reads

pytestmark = pytest.mark.gpu


def _totals(tot):
    return tot["lines"], tot["counted_tokens"], tot["a_tokens"], tot["long_lines"]


def _pack(container, data):
    return {"plain": lambda d: d, "gz": gzip.compress, "bgzf": lambda d: bgzf(d, block=30000)}[container](data)


@pytest.fixture(scope="module")
def regular():
    """600 KB inside the device's grammar with a long line, and what the reference makes of it"""
    rng = np.random.default_rng(23)
    data = random_text(rng, 300000) + long_line(LONG_LINE + 100) + random_text(rng, 234567)
    return data, kc.count(data)


@pytest.mark.parametrize("container", ["plain", "gz", "bgzf"])
@pytest.mark.parametrize("block", [4096 + 17, 65536, 0])
def test_files_against_the_helper(regular, tmp_path, monkeypatch, container, block):
    """blocks of 4113 and 65536 bytes: chunks are cut inside lines, and where the long line does not fit what a reader keeps in
    front of a block, the rest of the file goes line by line (one host chunk); 0: the default, one chunk"""
    data, (want_rows, want_tot) = regular
    if block:
        monkeypatch.setenv("GS_HOST_BLOCK_BYTES", str(block))
    path = str(tmp_path / ("in.out" + ("" if container == "plain" else ".gz")))
    open(path, "wb").write(_pack(container, data))
    csv = str(tmp_path / "res.csv")
    before = host.stat(5)
    rows, tot = host.kraken_count_files([path], csv=csv)
    assert rows == want_rows and _totals(tot) == tuple(want_tot.values())
    assert open(csv, "rb").read() == kc.csv(want_rows)
    assert tot["device_chunks"] == host.stat(5) - before >= (1 if block == 0 else 5)
    assert tot["host_chunks"] == 0 if block == 0 else tot["host_chunks"] <= 1


def test_refused_regions_and_the_tail(tmp_path, monkeypatch):
    """regions outside the grammar go through the line-by-line parser, chunk by chunk, and the device goes on behind them; the
    unterminated tail loses its last byte"""
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "32768")
    rng = np.random.default_rng(29)
    odd = [line(b"7:5 007:2", cls=b"007"), line(b"9:\x005"), line(b"9:5 3:1", desc=b"a b"), b"x\ty:3 4:2 \n"]
    parts = [random_text(rng, 100000)]
    for o in odd:
        parts += [o, random_text(rng, 100000)]
    data = b"".join(parts) + line(b"9:73")[:-1]
    want_rows, want_tot = kc.count(data)
    path = str(tmp_path / "in.out")
    open(path, "wb").write(data)
    before = host.stat(5)
    rows, tot = host.kraken_count_files([path])
    assert rows == want_rows and _totals(tot) == tuple(want_tot.values())
    assert tot["device_chunks"] == host.stat(5) - before > 0
    assert 4 <= tot["host_chunks"] <= 6  # (the four odd lines' chunks and the tail)
    monkeypatch.setenv("GS_HOST_FAST", "0")
    assert host.kraken_count_files([path])[0] == want_rows


def test_two_files_selection_and_empty_lines(regular, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    data, (rows_a, _) = regular
    second = random_text(np.random.default_rng(31), 90000) + b"\n" + line(b"9:1000000")  # its stream ends at the empty line
    rows_b, tot_b = kc.count(second)
    assert all(k != b"9" or v[1] < 1000000 for k, *v in rows_b)
    a, b = str(tmp_path / "a.out"), str(tmp_path / "b.out.gz")
    open(a, "wb").write(data)
    open(b, "wb").write(gzip.compress(second))
    merged = {}
    for k, *v in rows_a + rows_b + rows_a:
        merged[k] = [x + y for x, y in zip(merged.get(k, [0, 0, 0]), v)]
    want = [(k, *merged[k]) for k in sorted(merged)]
    csv = str(tmp_path / "res.csv.gz")
    rows, tot = host.kraken_count_files([a, b, a], csv=csv)
    assert rows == want and gzip.open(csv).read() == kc.csv(want)
    only = [b"562", b"0", b"424242"]
    rows, _ = host.kraken_count_files([a, b, a], only=only, csv=csv)
    assert rows == [r for r in want if r[0] in only] and len(rows) == 2
    assert gzip.open(csv).read() == kc.csv(rows)


def test_a_bad_file_fails_with_its_line(regular, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    data, _ = regular
    head = data[:data.index(b"\n", 400000) + 1]  # several chunks counted on the device in front of the bad line
    bad = head + line(b"9:5x") + data[len(head):]
    path, csv = str(tmp_path / "bad.out"), str(tmp_path / "res.csv")
    open(path, "wb").write(bad)
    with pytest.raises(ga.GsError) as e:
        host.kraken_count_files([path], csv=csv)
    assert e.value.args[0] == -1 or "line" in str(e.value)
    m = re.search(r"line (\d+):", str(e.value))
    assert m and int(m.group(1)) == head.count(b"\n") + 1 and "bad.out" in str(e.value)
    assert not os.path.exists(csv)
    with pytest.raises(kc.FormatError) as h:
        kc.count(bad)
    assert h.value.line == int(m.group(1))


@pytest.mark.parametrize("kind", ["fastq", "fasta"])
def test_round_trip_identities(tmp_path, kind):
    """a match run writes its Kraken-style lines on the device into a .gz; counted on the device, the file adds up to the run's
    own table: kmers and reads of every tax id (write_all on and off)"""
    sdb = synth.SynthDB(genera=2, species_per_genus=3, genome_len=20000, seed=13)
    store = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    recs = sample_reads(sdb.genomes, 20000, np.random.default_rng(41))
    if kind == "fastq":
        text = b"".join(d + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for d, r in recs)
    else:
        text = b"".join(b">" + d[1:] + b"\n" + r + b"\n" for d, r in recs)
    path = str(tmp_path / ("reads." + kind))
    open(path, "wb").write(text)
    try:
        for write_all in (True, False):
            kr = str(tmp_path / f"kraken{int(write_all)}.out.gz")
            on_device = host.stat(2) + host.stat(3)
            table, _, tot = host.match_files(store, [path], kraken_out_path=kr, taxids=sdb.taxids, write_all=write_all)
            assert host.stat(2) + host.stat(3) > on_device  # the lines were written on the device
            before = host.stat(5)
            rows, ktot = host.kraken_count_files([kr])
            assert host.stat(5) > before and ktot["host_chunks"] == 0
            check_identities(rows, table, sdb.taxids)
            n_class = int(table[:, 0].sum())
            assert 0 < n_class < len(recs) and ktot["a_tokens"] > 0
            assert ktot["lines"] == (sum(len(r) >= 31 for _, r in recs) if write_all else n_class)
            assert rows == kc.count(gzip.open(kr).read())[0]
    finally:
        store.close()
