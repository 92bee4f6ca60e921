"""host.match_files with Kraken-style output: the lines of four-line chunks are written on the device (gs_match_kraken_text behind a
DeviceWriter of their own) -- for plain and gzip input, plain and .gz outputs, with and without a filtered file beside them, with
write_all on and off.  The text must equal the plain-Python rule of tests/krakenlines.py over the oracle's classes, the filtered
file the reads the oracle returns, GS_DEVICE_KRAKEN=0 (the host formatter) must give the same text, and gs_host_stat(2) says which
of the two ran.  Chunks that do not qualify keep the host formatter, in read order.  Needs an MI355X: run with -m gpu."""
import gzip
import itertools

import numpy as np
import pytest

import genestrip_amd as ga
import krakenlines
import matchcheck
from genestrip_amd import host, synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

N = 5000


@pytest.fixture(scope="module")
def sdb():
    return synth.SynthDB(genera=2, species_per_genus=3, genome_len=20000, seed=7)


@pytest.fixture(scope="module")
def store(sdb):
    s = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    yield s
    s.close()


@pytest.fixture(scope="module")
def odb(sdb):
    return orc.DB(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)


def _expected(odb, taxids, data, fasta=False):
    """(lines with write_all, lines without, filtered text) of a file's bytes, through the reference parser and the oracle"""
    p = orc.parse_fastq(data, fasta=fasta, k=31)
    n = int(p["n_reads"])
    seq = p["seq"] if len(p["seq"]) else np.zeros(1, dtype=np.uint8)
    o = matchcheck.oracle_batch(odb, seq, p["seq_off"])
    field = lambda name, i: bytes(p[name][int(p[name + "_off"][i]):int(p[name + "_off"][i + 1])])
    segs = {}
    out = {True: [], False: []}
    filtered = []
    for i in range(n):
        d, s = field("desc", i), field("seq", i)
        if s not in segs:
            segs[s] = odb.segments(s) if len(s) >= 31 else []
        for wa in (True, False):
            out[wa].append(krakenlines.line(d, len(s), 31, segs[s], int(o["class_vi"][i]), taxids, wa))
        if o["flags"][i] & orc.F_RETURNED:
            filtered.append(d + b"\n" + s + b"\n+\n" + b"~" * len(s) + b"\n")
    return b"".join(out[True]), b"".join(out[False]), b"".join(filtered)


@pytest.fixture(scope="module")
def sample(sdb, odb):
    seq, off = synth.reads_host(sdb.genomes, N, read_len=150, seed=31)
    seq = seq.copy()
    rng = np.random.default_rng(3)
    for i in range(0, N, 4):  # a quarter of the reads hit nothing: lines that write_all = 0 leaves out
        seq[150 * i:150 * (i + 1)] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 150)]
    seq[150 * 5 + 70] = ord("N")
    seq[150 * 3006:150 * 3006 + 3] = ord("N")
    data = b"".join(b"@r%d sample=%d\n" % (i, i % 7) + seq[150 * i:150 * (i + 1)].tobytes() + b"\n+\n" + b"I" * 150 + b"\n" for i in range(N))
    return data, _expected(odb, sdb.taxids, data)


def _read(path):
    return gzip.open(path).read() if str(path).endswith(".gz") else open(path, "rb").read()


@pytest.mark.parametrize("in_gz,kr_gz", list(itertools.product((False, True), (False, True))))
def test_kraken_lines_of_files_on_the_device(sdb, store, sample, tmp_path, monkeypatch, in_gz, kr_gz):
    data, (want_all, want_classified, want_filtered) = sample
    assert 0 < len(want_classified) < len(want_all) and want_all.count(b"\n") == N and b" A:" in want_all and want_filtered
    path = str(tmp_path / ("in.fastq.gz" if in_gz else "in.fastq"))
    with (gzip.open(path, "wb", compresslevel=1) if in_gz else open(path, "wb")) as f:
        f.write(data)
    for with_filtered, write_all in itertools.product((False, True), (False, True)):
        for device in (True, False):
            if device:
                monkeypatch.delenv("GS_DEVICE_KRAKEN", raising=False)
            else:
                monkeypatch.setenv("GS_DEVICE_KRAKEN", "0")
            tag = f"{int(with_filtered)}{int(write_all)}{int(device)}"
            kr = str(tmp_path / ("k" + tag + (".out.gz" if kr_gz else ".out")))
            fl = str(tmp_path / ("f" + tag + (".fastq.gz" if kr_gz else ".fastq"))) if with_filtered else None
            before = host.stat(2)
            _, _, tot = host.match_files(store, [path], kraken_out_path=kr, filtered_path=fl, taxids=sdb.taxids, write_all=write_all)
            grew = host.stat(2) - before
            what = (in_gz, kr_gz, with_filtered, write_all, device)
            assert tot.reads == N, what
            assert _read(kr) == (want_all if write_all else want_classified), what
            if with_filtered:
                assert _read(fl) == want_filtered, what
                assert tot.filtered_reads == want_filtered.count(b"\n") // 4, what
            assert (grew > 0) == device, (what, grew)  # the lines came from the device, or (GS_DEVICE_KRAKEN=0) from the host formatter


def test_fasta_file_keeps_the_host_formatter(sdb, store, odb, tmp_path):
    g = sdb.genomes
    data = b"".join(b">contig%d some text\n" % i + bytes(g[i % len(g), 300 * i:300 * i + 400]) + b"\n" + bytes(g[i % len(g), 50:120]) + b"\n" for i in range(40))
    want_all, _, _ = _expected(odb, sdb.taxids, data, fasta=True)
    path = str(tmp_path / "in.fasta")
    open(path, "wb").write(data)
    kr = str(tmp_path / "k.out")
    before = host.stat(2)
    _, _, tot = host.match_files(store, [path], kraken_out_path=kr, taxids=sdb.taxids)
    assert tot.reads == 40 and _read(kr) == want_all and want_all.count(b"\n") == 40
    assert host.stat(2) == before


@pytest.mark.parametrize("kr_gz", [False, True])
def test_device_chunks_then_a_tail_for_the_parser_stay_in_read_order(sdb, store, odb, sample, tmp_path, monkeypatch, kr_gz):
    data, _ = sample
    data = data[:150 * 1024 * 2 + 317]
    data = data[:data.rfind(b"\n@r") + 1]  # whole records ...
    data = data[:-1]                         # ... but the last one without its final newline: the cutter leaves it to the parser
    want_all, _, want_filtered = _expected(odb, sdb.taxids, data)
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")  # several device chunks in front of the tail
    path = str(tmp_path / "tail.fastq")
    open(path, "wb").write(data)
    kr = str(tmp_path / ("k.out.gz" if kr_gz else "k.out"))
    fl = str(tmp_path / ("f.fastq.gz" if kr_gz else "f.fastq"))
    before = host.stat(2)
    _, _, tot = host.match_files(store, [path], kraken_out_path=kr, filtered_path=fl, taxids=sdb.taxids)
    assert host.stat(2) - before >= 2
    assert tot.reads == want_all.count(b"\n")
    assert _read(kr) == want_all
    assert _read(fl) == want_filtered
