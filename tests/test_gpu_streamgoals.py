"""extract and fasta2fastq on the device: gs_reads_fasta2fastq, the three gs_reads_select_* calls with gs_reads_compact_text, and
both goals file by file (gs_host_extract_files, gs_host_fasta2fastq), byte-equal to the two Java loops restated in
tests/streamgoals.py.  Small shapes: every lane, tile and block edge of the kernels, nothing of the workload's size -- the second
level of the block scans (more than 262 144 lines or records, text beyond 64 MiB, output beyond the copy grid) is the subject of
tests/test_gpu_chunk_scale.py."""
import gzip
import os

import numpy as np
import pytest

import genestrip_amd as ga
import streamgoals as sg
from conftest import GOLDEN, bgzf
from genestrip_amd import host

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "fasta2fastq", "fasta2fastqtest.fasta")


@pytest.fixture(scope="module")
def reads():
    r = ga.DeviceReads(k=5)
    yield r
    r.close()


def bases(n, seed):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def record(name, line_lens, seed, eol=b"\n"):
    return b">" + name + eol + b"".join(bases(n, seed + i) + eol for i, n in enumerate(line_lens))


def f2f_chunks():
    small = b"".join(record(b"r%d" % i, [20], i) for i in range(40))
    return {
        "fixture": open(FIXTURE, "rb").read(),
        # lane and 4096-byte tile edges of the newline scan and of the copy
        "line lengths": b"".join(record(b"len%d x" % n, [n, 1, n], n) for n in (1, 63, 64, 65, 4095, 4096, 4097)),
        # GS_FA_BLOCK lines per block of the per-line scan
        "lines per record": b"".join(record(b"lines%d" % n, [3] * n, n) for n in (255, 256, 257, 254)),
        "a header as the last line": record(b"a", [10, 7], 1) + b">last one\n",
        "crlf and empty lines": b">h1 x\r\nACGT\r\nAC\r\r\n\nGG\n\r\n>h2\r\r\nT\n\n\n>h3\n" + record(b"w", [70, 70, 3], 2, b"\r\n"),
        # a piece of the copy spans many records, one record spans many pieces
        "one long record": small + record(b"chromosome 1", [60] * 5000, 7) + small,
        "no sequence at all": b">a\n>b\n\n>c\n\r\n\r\r\n>d e f\n",
    }


F2F = f2f_chunks()


@pytest.mark.parametrize("name", sorted(F2F))
def test_fasta2fastq_chunk(reads, name):
    data = F2F[name]
    want, _ = sg.fasta2fastq(data)
    reads.text_reset(True)
    for slot in (0, 1):
        got, long_lines = reads.fasta2fastq(data, slot=slot)
        assert long_lines == 0 and reads.text_status()[0] == -1
        assert got.tobytes() == want


def test_fasta2fastq_refusals_and_long_line(reads):
    ok = b">a\nACGT\n"
    for bad in (b">a\nAC\0GT\n", b"ACGT\n>a\nAC\n", b"\n>a\nAC\n"):
        reads.text_reset(True)
        got, _ = reads.fasta2fastq(bad)
        failed, _, totals = reads.text_status()
        assert len(got) == 0 and failed >= 0 and totals[0] == 0, bad
        got, _ = reads.fasta2fastq(ok)  # (the refusal is sticky, as for match and filter)
        assert len(got) == 0
    reads.text_reset(True)
    for n_lines, n_records in ((3, 1), (2, 2)):  # wrong counts
        got, _ = reads.fasta2fastq(ok, n_lines=n_lines, n_records=n_records)
        assert len(got) == 0 and reads.text_status()[0] >= 0
        reads.text_reset(True)
    # the reference throws from 65 534 bytes incl. the newline: flagged, not refused
    for n, flagged in ((65532, 0), (65533, 1)):
        data = b">a\n" + b"A" * n + b"\nCC\n"
        got, long_lines = reads.fasta2fastq(data)
        assert long_lines == flagged and reads.text_status()[0] == -1
        assert got.tobytes() == b"@a\n" + b"A" * n + b"CC\n+\n" + b"~" * (n + 2) + b"\n"
    assert reads.text_status()[2][0] == 2  # records of the accepted chunks since the last reset


def fastq_chunk(n, seed, eol=b"\n"):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(1, 90))
        out.append(b"@s%d/%d run%d" % (i % 3, i, seed) + eol + bases(L, seed * 1000 + i) + eol + b"+" + eol + b"I" * L + eol)
    return out


def test_extract_four_line_chunk(reads):
    recs = [b"@s0 first\nACGT\n+\nIIII\n"] + fastq_chunk(700, 3) + [b"@s\nAC\n+\nII\n"] + fastq_chunk(40, 9) + [b"@s-last 1\nA\n+\nI\n"]
    data = b"".join(recs)
    # a key of one byte (every record), whole descriptors at both ends of the chunk, one byte more than the shortest descriptor, none
    counts = {b"s": len(recs), b"s0 first": 1, b"s-last 1": 1, b"s0": None, b"s1/1 run3": 1, b"s-last 12": 0, b"none": 0}
    for key, count in counts.items():
        reads.text_reset(True)
        acc = reads.select_text(data, key)
        want, n = sg.extract(data, key)
        assert int(acc.sum()) == n and (count is None or n == count), key
        for probs in (True, False):
            got, nr = reads.compact_text(with_probs=probs, slot=int(probs))
            assert nr == n
            assert got.tobytes() == (want if probs else sg.extract(data, key, with_probs=False)[0]), (key, probs)


def test_extract_chunk_without_records(reads):
    # nothing to flag, nothing to write: 0 bytes and 0 records, not a state error -- whatever chunk the handle saw before
    reads.text_reset(True)
    data = b"".join(fastq_chunk(5, 2))
    assert int(reads.select_text(data, b"s").sum()) == 5
    for select in (reads.select_text, reads.select_fasta):
        assert len(select(b"", b"s")) == 0
        got, nr = reads.compact_text()
        assert (len(got), nr) == (0, 0)
    assert reads.text_status()[0] == -1
    assert int(reads.select_text(data, b"s").sum()) == 5 and reads.compact_text()[0].tobytes() == data


def test_extract_crlf_descriptor(reads):
    data = b"".join(fastq_chunk(50, 4, b"\r\n"))
    for key in (b"s1/1 run4\r", b"s1/1 run4", b"s1/1 run4\r\n"):
        reads.text_reset(True)
        acc = reads.select_text(data, key)
        want, n = sg.extract(data, key)
        got, nr = reads.compact_text()
        assert (int(acc.sum()), nr, got.tobytes()) == (n, n, want), key
    assert sg.extract(data, b"s1/1 run4\r")[1] == 1 and sg.extract(data, b"s1/1 run4\r\n")[1] == 0


def test_extract_fasta_chunk(reads):
    data = F2F["one long record"] + record(b"r0", [1], 5) + F2F["lines per record"] + record(b"r3 last", [64, 64], 6, b"\r\n")
    first = data[1:data.index(b"\n")]
    for key in (b"r", b"r3", b"chromosome 1", b"chromosome 10", first, b"r3 last\r", b"zzz", b"l"):
        reads.text_reset(True)
        acc = reads.select_fasta(data, key)
        want, n = sg.extract(data, key, fasta=True)
        got, nr = reads.compact_text()
        assert (int(acc.sum()), nr) == (n, n), key
        assert got.tobytes() == want, key
    assert sg.extract(data, b"zzz", fasta=True)[1] == 0 and sg.extract(data, b"r3 last\r", fasta=True)[1] == 1


def test_read_entry_mode_keeps_cr_goal_mode_does_not(reads):
    data = b">a\r\nAC\r\nGT\r\n>b\r\nT\r\n"
    reads.text_reset(True)
    assert int(reads.select_fasta(data, b"a").sum()) == 1 and int(reads.select_fasta(data, b"b\r").sum()) == 1
    reads.select_fasta(data, b"a")
    got, _ = reads.compact_text()
    assert got.tobytes() == b"@a\r\nAC\rGT\r\n+\n~~~~~~\n" == sg.extract(data, b"a", fasta=True)[0]
    got, _ = reads.fasta2fastq(data)
    assert got.tobytes() == b"@a\r\nACGT\n+\n~~~~\n@b\r\nT\n+\n~\n" == sg.fasta2fastq(data)[0]


def test_select_general_fastq_and_refusals(reads):
    data = b"@m1 x\nACGT\nAC\n+\nIIII\nII\n@n2\nGG\n+\nII\n@m3\nT\n+\nI\n"
    reads.text_reset(True)
    n_rec, used, acc = reads.select_fastq_ml(data, b"m")
    assert (n_rec, used, acc.tolist()) == (3, len(data), [1, 0, 1])
    with pytest.raises(ga.GsError) as e:  # written by the host's writers, as the filter goal does
        reads.compact_text()
    assert e.value.code == -4
    # a chunk that is not four lines per record: refused exactly as the filter's, flags all zero
    reads.text_reset(True)
    acc = reads.select_text(data[:data.index(b"@n2")] + b"x\ny\n", b"m")
    assert reads.text_status()[0] >= 0 and int(acc.sum()) == 0
    reads.text_reset(True)
    for key in (b"", b"a\0b", b"a\xc3"):
        with pytest.raises(ga.GsError) as e:
            reads.select_text(b"@a\nAC\n+\nII\n", key)
        assert e.value.code == -1


# ---- file level ----
def small_fasta(n, seed):
    return b"".join(record(b"q%d" % i, [12, 5], seed + i) for i in range(n))


def write_inputs(tmp_path, kind, name, data):
    p = tmp_path / (name + {"plain": "", "gzip": ".gz", "bgzf": ".gz"}[kind])
    p.write_bytes({"plain": data, "gzip": gzip.compress(data), "bgzf": bgzf(data)}[kind])
    return p


def read_out(p):
    raw = p.read_bytes()
    return gzip.decompress(raw) if p.name.endswith(".gz") else raw


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
def test_fasta2fastq_files(tmp_path, monkeypatch, kind):
    datas = [F2F["one long record"] + F2F["crlf and empty lines"], small_fasta(300, 11) + b">tail without newline\nACGT"]
    paths = [write_inputs(tmp_path, kind, "in%d.fasta" % i, d) for i, d in enumerate(datas)]
    want = sg.fasta2fastq_files(datas)
    n = sum(sg.fasta2fastq(d)[1] for d in datas)
    outs = {}
    for mode, env in (("device", {}), ("blocks", {"GS_HOST_BLOCK_BYTES": "64"}), ("cpu", {"GS_HOST_FAST": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for out_name in ("o.fastq.gz", "o.fastq"):
            dst = tmp_path / (mode + out_name)
            assert host.fasta2fastq(paths, dst) == n
            outs[mode, out_name] = read_out(dst)
        for k in env:
            monkeypatch.delenv(k)
    assert all(o == want for o in outs.values()), [k for k, o in outs.items() if o != want]


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
def test_extract_files(tmp_path, monkeypatch, kind):
    ml = b"".join(b"@s%d ml\nACGTAC\nGT\n+\nIIIIII\nII\n" % i for i in range(40))
    datas = [(b"".join(fastq_chunk(900, 21)), "a.fastq", False), (small_fasta(300, 5).replace(b">q1", b">s1"), "b.fasta", True), (ml, "c.fastq", False)]
    paths = [write_inputs(tmp_path, kind, name, d) for d, name, _ in datas]
    bloom = ga.DeviceBloomFilter(ga.BLOOM_XOR, 64, [1], np.zeros(1, np.uint64))
    ftot = host.filter_files(bloom, 5, paths)
    for key in (b"s1", b"s"):
        parts = [sg.extract(d, key, fasta=fa) for d, _, fa in datas]
        want, n = b"".join(p[0] for p in parts), sum(p[1] for p in parts)
        assert n > 0
        for mode, env in (("device", {}), ("blocks", {"GS_HOST_BLOCK_BYTES": "64"}), ("cpu", {"GS_HOST_FAST": "0"})):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            for out_name in ("o.fastq.gz", "o.fastq"):
                dst = tmp_path / (mode + out_name)
                tot = host.extract_files(key, paths, dst, k=5)
                assert read_out(dst) == want, (key, mode, out_name)
                assert (tot.filtered_reads, tot.reads, tot.kmers, tot.bps) == (n, ftot.reads, ftot.kmers, ftot.bps), (key, mode)
            for k in env:
                monkeypatch.delenv(k)
