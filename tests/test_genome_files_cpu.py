"""host.genome_files without a GPU: under GS_HOST_FAST=0 every file goes through the line-by-line parser of the host layer
(genestrip_amd/csrc/gs_genomeparse.h) and no device is used, so the walk, the resolve / sink callbacks and the totals can be held
to the plain restatement (tests/genomefasta.py) here.  The device path has the same tests in tests/test_gpu_genome_files.py."""
import gzip

import numpy as np
import pytest

import genestrip_amd as ga
import genomefasta as gf
from genestrip_amd import host
from genomefasta_cases import CASES


@pytest.fixture(autouse=True)
def _host_only(monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")


def _walk(paths, resolve=None):
    got = {"headers": [], "seq": [], "off": [0], "vi": [], "calls": []}

    def _resolve(file, first, headers):
        got["calls"].append((file, first, len(headers)))
        got["headers"] += headers
        return resolve(headers) if resolve else [0] * len(headers)

    def _sink(seq, off, vi):
        assert isinstance(seq, np.ndarray) and len(off) == len(vi) + 1 and off[0] == 0
        got["seq"].append(bytes(seq))
        got["off"] += [got["off"][-1] + int(x) for x in off[1:]]
        got["vi"] += vi.tolist()

    got["totals"] = host.genome_files(paths, _resolve, _sink)
    got["seq"] = b"".join(got["seq"])
    return got


@pytest.mark.parametrize("case", [c for c in CASES if c[2]], ids=[c[0] for c in CASES if c[2]])
def test_hand_written_streams_as_files(tmp_path, case):
    _, data, _, headers, seq, offsets, max_line, _ = case
    path = tmp_path / "x.fasta"
    path.write_bytes(data)
    got = _walk([path])
    assert (got["headers"], got["seq"]) == (headers, seq)
    if headers:  # (a file without records never reaches the sink)
        assert got["off"] == offsets
    t = got["totals"]
    assert (t.records, t.kept_records, t.kept_bases, t.max_line_bytes) == (len(headers), len(headers), len(seq), max_line)
    assert t.host_chunks == t.chunks


def test_files_in_order_with_a_resolver_that_skips(tmp_path):
    rng = np.random.default_rng(3)
    files, want_h, want_parts = [], [], []
    for f in range(3):
        recs = []
        for i in range(7):
            body = bytes(rng.choice(np.frombuffer(b"ACGTn", np.uint8), int(rng.integers(0, 300))))
            eol = b"\r\n" if (f + i) % 3 == 0 else b"\n"
            recs.append(b">f%d_%d" % (f, i) + eol + b"".join(body[j:j + 50] + eol for j in range(0, len(body), 50)))
        data = b"".join(recs)
        path = tmp_path / ("g%d.fasta%s" % (f, ".gz" if f == 1 else ""))
        path.write_bytes(gzip.compress(data) if f == 1 else data)
        files.append(path)
        headers, seq, off, _, _ = gf.read_fasta(data)
        want_h += headers
        want_parts += [seq[off[i]:off[i + 1]] for i in range(7)]
    rule = lambda h: -1 if h.endswith(b"3") else int(h[-1:])  # (of the header line without its '\r')
    got = _walk(files, lambda headers: [rule(h.rstrip()) for h in headers])
    keep = [not h.rstrip().endswith(b"3") for h in want_h]
    assert got["headers"] == want_h
    assert got["seq"] == b"".join(p for p, k in zip(want_parts, keep) if k)
    assert got["vi"] == [rule(h.rstrip()) for h, k in zip(want_h, keep) if k]
    assert [c[0] for c in got["calls"]] == [0, 1, 2] and all(c[1] == 0 for c in got["calls"])
    assert got["totals"].records == 21 and got["totals"].kept_records == 18


def test_record_of_many_buffers_is_walked_once(tmp_path):
    """the line-by-line loop reads some MiB at a time and cuts in front of the last header line it has seen: a record of 13 MB
    (wrapped) and one of 9 MB (one line) between small ones come out as the restatement has them"""
    rng = np.random.default_rng(8)
    body = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    big = body(13_000_000)
    data = (b"in front\n>s0\n" + body(100) + b"\n>big wrapped\n" + b"".join(big[j:j + 80] + b"\r\n" for j in range(0, len(big), 80)) +
            b">s1\n" + body(50) + b"\n>big line\n" + body(9_000_000) + b"\n>s2\nAC\n>s3\n" + body(7) )
    path = tmp_path / "big.fasta.gz"
    path.write_bytes(gzip.compress(data, 1))
    got = _walk([path], lambda headers: [0 if h != b">s1" else -1 for h in headers])
    headers, seq, off, max_line, _ = gf.read_fasta(data)
    assert got["headers"] == headers == [b">s0", b">big wrapped", b">s1", b">big line", b">s2", b">s3"]
    assert got["seq"] == b"".join(seq[off[i]:off[i + 1]] for i in range(6) if i != 2)
    assert [c[1] for c in got["calls"]] == list(np.cumsum([0] + [c[2] for c in got["calls"]])[:-1])
    t = got["totals"]
    assert (t.records, t.kept_records, t.max_line_bytes) == (6, 5, max_line) and t.chunks >= 3


def test_callback_codes_and_exceptions_end_the_walk(tmp_path):
    path = tmp_path / "x.fasta"
    path.write_bytes(b">a\nACGT\n>b\nGG\n")
    sunk = []
    with pytest.raises(ga.GsError) as e:
        host.genome_files([path, path], lambda f, first, headers: 77, lambda s, o, v: sunk.append(1))
    assert e.value.code == 77 and not sunk
    with pytest.raises(ga.GsError) as e:
        host.genome_files([path], lambda f, first, headers: [0, 1], lambda s, o, v: 31)
    assert e.value.code == 31
    with pytest.raises(KeyError):
        host.genome_files([path], lambda f, first, headers: {}["no such accession"], lambda s, o, v: None)
    with pytest.raises(ValueError):
        host.genome_files([path], lambda f, first, headers: [0], lambda s, o, v: None)
    with pytest.raises(ga.GsError) as e:
        host.genome_files([tmp_path / "missing.fasta"], lambda f, first, headers: [0] * len(headers), lambda s, o, v: None)
    assert e.value.code == -7
    assert host.lib().gs_host_genome_files(None, 0, 0, None, None, None, None, None) == -1
