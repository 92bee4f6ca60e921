"""The file loops over FASTA and wrapped-FASTQ files with per-read outputs: host.match_files (Kraken-style lines, filtered file),
host.filter_files (accepted and rest file) and host.extract_files write the records of such chunks on the device
(gs_*_compact_records, gs_match_kraken_records behind the DeviceWriters); GS_DEVICE_RECORDS=0 keeps them on the host formatter.
Both ways must give the oracle-based expectation byte for byte (.gz after inflating), gs_host_stat(3) says which of the two ran,
gs_host_stat(2) stays with the four-line chunks.  Blocks of 64 KiB: several chunks and carries per file.
Needs an MI355X: run with -m gpu."""
import gzip

import numpy as np
import pytest

import genestrip_amd as ga
import recordtext as rt
import streamgoals
from genestrip_amd import host, synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

N = 420


@pytest.fixture(scope="module")
def sdb():
    return synth.SynthDB(genera=2, species_per_genus=3, genome_len=20000, seed=7)


@pytest.fixture(scope="module")
def side(sdb):
    s = rt.Side(ga, 31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    yield s
    s.close()


@pytest.fixture(scope="module")
def blooms(sdb):
    keys = sdb.kmers[np.isin(sdb.value_idx, sdb.species_vi)]
    ob = orc.Bloom(orc.BLOOM_XOR, len(keys), 1e-8)
    ob.put_many(keys)
    return ga.DeviceBloomFilter(ga.BLOOM_XOR, ob.bits, ob.hash_factors, ob.words), ob


@pytest.fixture(scope="module")
def files(sdb, side, blooms):
    """a FASTA and a wrapped-FASTQ file of N records each (a quarter of the reads random, one with an 'N', some short, FASTA records
    without a sequence) and everything the goals are expected to write for them, computed once"""
    seq, off = synth.reads_host(sdb.genomes, N, read_len=150, seed=31)
    rng = np.random.default_rng(3)
    reads = []
    for i in range(N):
        r = bytes(seq[150 * i:150 * (i + 1)])
        if i % 4 == 0:
            r = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 150))
        if i == 5:
            r = r[:70] + b"N" + r[71:]
        if i % 50 == 7:
            r = r[:25]  # shorter than k
        reads.append(r)
    desc = lambda i: (b"K%d sample=%d" if i % 3 else b"Z%d other %d") % (i, i % 7)
    qual = lambda n: bytes(b"IJKL#~5"[x] for x in rng.integers(0, 7, n))
    fa = rt.fasta([(b">" + desc(i), b"" if i % 97 == 13 else reads[i] + (reads[(i + 1) % N] if len(reads[i]) == 150 else b"")) for i in range(N)], 60)
    fq = rt.fastq_ml([(b"@" + desc(i), reads[i], qual(len(reads[i]) + (4 if i % 5 == 0 else 0)), 1 + i % 3, 1 + (i // 3) % 3) for i in range(N)])
    _, ob = blooms
    out = {}
    for name, data, is_fasta in (("fasta", fa, True), ("fastq", fq, False)):
        ents = rt.entries(data, is_fasta)
        assert len(ents) == N and len(data) > 65536 * 3 // 2  # (two chunks at least)
        rs = [r for _, r, _ in ents]
        cv, fl = side.match(rs)
        ret = (fl & orc.F_RETURNED) != 0
        s, o = orc.pack_reads(rs)
        acc = ob.filter_batch(31, 1, 0.2, s, o).astype(bool)
        out[name] = dict(data=data, ents=ents,
                         kraken={wa: rt.kraken_text(ents, 31, side.segments, cv, sdb.taxids, wa) for wa in (True, False)},
                         filtered={p: rt.record_text(ents, ret, p) for p in (True, False)},
                         accepted={p: rt.record_text(ents, acc, p) for p in (True, False)},
                         rest={p: rt.record_text(ents, ~acc, p) for p in (True, False)},
                         extract=streamgoals.extract(data, b"K", is_fasta), n_acc=int(acc.sum()), n_ret=int(ret.sum()))
        assert 0 < acc.sum() < N and 0 < ret.sum() < N and 0 < out[name]["extract"][1] < N
    return out


def _read(path):
    return gzip.open(path).read() if str(path).endswith(".gz") else open(path, "rb").read()


def _write(tmp_path, name, data):
    path = str(tmp_path / name)
    open(path, "wb").write(data)
    return path


def _ways(monkeypatch):
    """(device path?, tag) twice: the device path, then GS_DEVICE_RECORDS=0"""
    for device in (True, False):
        if device:
            monkeypatch.delenv("GS_DEVICE_RECORDS", raising=False)
        else:
            monkeypatch.setenv("GS_DEVICE_RECORDS", "0")
        yield device, "d" if device else "h"


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
@pytest.mark.parametrize("gz", [False, True])
def test_match_files(sdb, side, files, tmp_path, monkeypatch, kind, gz):
    w = files[kind]
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    path = _write(tmp_path, "in." + kind, w["data"])
    ext = ".gz" if gz else ""
    for write_all, with_filtered in ((True, True), (False, False)):
        for device, tag in _ways(monkeypatch):
            kr = str(tmp_path / f"k{tag}{int(write_all)}.out{ext}")
            fl = str(tmp_path / f"f{tag}{int(write_all)}.fastq{ext}") if with_filtered else None
            b2, b3 = host.stat(2), host.stat(3)
            _, _, tot = host.match_files(side.store, [path], kraken_out_path=kr, filtered_path=fl, taxids=sdb.taxids, write_all=write_all)
            what = (kind, gz, write_all, device)
            assert _read(kr) == w["kraken"][write_all], what
            if with_filtered:
                assert _read(fl) == w["filtered"][False], what
                assert tot.filtered_reads == w["n_ret"], what
            assert host.stat(2) == b2, what
            assert (host.stat(3) - b3 >= 2) if device else (host.stat(3) == b3), (what, host.stat(3) - b3)


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
def test_match_files_filtered_alone_with_qualities(sdb, side, files, tmp_path, monkeypatch, kind):
    w = files[kind]
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    path = _write(tmp_path, "in." + kind, w["data"])
    for device, tag in _ways(monkeypatch):
        fl = str(tmp_path / f"f{tag}.fastq.gz")
        b3 = host.stat(3)
        _, _, tot = host.match_files(side.store, [path], filtered_path=fl, taxids=sdb.taxids, with_probs=True)
        assert _read(fl) == w["filtered"][True] and tot.filtered_reads == w["n_ret"], (kind, device)
        assert (host.stat(3) > b3) == device


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
@pytest.mark.parametrize("gz", [False, True])
def test_filter_files(blooms, files, tmp_path, monkeypatch, kind, gz):
    w = files[kind]
    bloom, _ = blooms
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    path = _write(tmp_path, "in." + kind, w["data"])
    ext = ".gz" if gz else ""
    for probs in (True, False):
        for device, tag in _ways(monkeypatch):
            a = str(tmp_path / f"a{tag}{int(probs)}.fastq{ext}")
            r = str(tmp_path / f"r{tag}{int(probs)}.fastq{ext}")
            b2, b3 = host.stat(2), host.stat(3)
            tot = host.filter_files(bloom, 31, [path], filtered_path=a, rest_path=r, with_probs=probs)
            what = (kind, gz, probs, device)
            assert tot.filtered_reads == w["n_acc"], what
            assert _read(a) == w["accepted"][probs], what
            assert _read(r) == w["rest"][probs], what
            assert host.stat(2) == b2, what
            # (plain outputs of a plain file are formatted from the reader's block, as for four-line chunks)
            assert (host.stat(3) - b3 >= 2) if (device and gz) else (host.stat(3) == b3), (what, host.stat(3) - b3)


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
@pytest.mark.parametrize("gz", [False, True])
def test_extract_files(files, tmp_path, monkeypatch, kind, gz):
    w = files[kind]
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    path = _write(tmp_path, "in." + kind, w["data"])
    want, n_want = w["extract"]
    for device, tag in _ways(monkeypatch):
        out = str(tmp_path / (f"x{tag}.fastq" + (".gz" if gz else "")))
        b2, b3 = host.stat(2), host.stat(3)
        tot = host.extract_files(b"K", [path], out)
        assert tot.filtered_reads == n_want, (kind, gz, device)
        assert _read(out) == want, (kind, gz, device)
        assert host.stat(2) == b2
        assert (host.stat(3) - b3 >= 2) if (device and gz) else (host.stat(3) == b3), (kind, gz, device, host.stat(3) - b3)


def test_four_line_chunks_then_a_wrapped_tail_stay_in_read_order(sdb, side, blooms, files, tmp_path, monkeypatch):
    """four-line records for three blocks, then wrapped records: the outputs of the chunks the device wrote and of what follows them
    come in read order"""
    ents = files["fastq"]["ents"]
    head = b"".join(d + b"\n" + r + b"\n+\n" + q[:len(r)] + b"\n" for d, r, q in ents[:N - 60])
    tail = files["fastq"]["data"]
    tail = tail[tail.index(ents[N - 60][0] + b"\n"):]
    data = head + tail
    all_ents = rt.entries(data, False)
    assert len(all_ents) == N and len(head) > 65536 * 3 // 2  # (a whole block of four-line records in front of the tail)
    rs = [r for _, r, _ in all_ents]
    cv, fl = side.match(rs)
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    path = _write(tmp_path, "mixed.fastq", data)
    kr, fo = str(tmp_path / "k.out.gz"), str(tmp_path / "f.fastq.gz")
    host.match_files(side.store, [path], kraken_out_path=kr, filtered_path=fo, taxids=sdb.taxids)
    assert _read(kr) == rt.kraken_text(all_ents, 31, side.segments, cv, sdb.taxids, True)
    assert _read(fo) == rt.record_text(all_ents, (fl & orc.F_RETURNED) != 0, False)
    bloom, ob = blooms
    s, o = orc.pack_reads(rs)
    acc = ob.filter_batch(31, 1, 0.2, s, o).astype(bool)
    a, r = str(tmp_path / "a.fastq.gz"), str(tmp_path / "r.fastq.gz")
    host.filter_files(bloom, 31, [path], filtered_path=a, rest_path=r, with_probs=True)
    assert _read(a) == rt.record_text(all_ents, acc, True) and _read(r) == rt.record_text(all_ents, ~acc, True)
    x = str(tmp_path / "x.fastq.gz")
    host.extract_files(b"K", [path], x)
    assert _read(x) == streamgoals.extract(data, b"K", False)[0]
