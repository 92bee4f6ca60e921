"""The krakencount goal without a device: the plain-Python restatement of the reference (tests/krakencount.py) against cases worked
out by hand and against the one reference-held vector; the host layer's line-by-line parser (GS_HOST_FAST=0) against it, on the
cases and on files in every container format; the two identities that tie a Kraken-style file to its run's table, on the oracle;
the parser on its own under AddressSanitizer."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import genestrip_amd as ga
import krakencount as kc
import krakenlines
import matchcheck
from conftest import GOLDEN, bgzf
from genestrip_amd import host, synth
from krakencount_cases import CASES, LONG_LINE, check_identities, line, long_line, random_text, sample_reads
from oracle import gs_oracle as orc


def _count(case, **kw):
    try:
        rows, tot = kc.count(case.data, case.only, **kw)
        return rows, (tot["lines"], tot["counted"], tot["a_tokens"])
    except kc.FormatError as e:
        return ("error", e.line), None


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_helper_on_hand_written_cases(case):
    for fast in (True, False):
        assert _count(case, fast=fast) == (case.expect, case.totals)
    # the device's grammar, as the helper states it, takes exactly the cases marked for it
    lines = case.data.split(b"\n")
    body = lines[:-1]
    if b"" in body:
        body = body[:body.index(b"")]
    inside = case.data.endswith(b"\n") and all(kc.in_grammar(l) for l in body)
    assert inside == (case.bad_line is None)
    if case.bad_line is not None and case.data.endswith(b"\n"):
        assert [kc.in_grammar(l) for l in body].index(False) == case.bad_line


def test_helper_on_the_golden_line():
    data = open(os.path.join(GOLDEN, "dengue1", "test.out"), "rb").read()
    rows, tot = kc.count(data)
    assert rows == [(b"0", 0, 4, 0), (b"1", 1, 7, 0)] and tot == {"lines": 1, "counted": 3, "a_tokens": 0, "long_lines": 0}
    assert kc.csv(rows) == b"taxid;reads;kmers;kmers in matching reads\n0;0;4;0;\n1;1;7;0;\n"


def test_helper_long_lines_both_ways():
    ok, over = long_line(LONG_LINE), long_line(LONG_LINE + 1)
    assert len(ok) == LONG_LINE and len(over) == LONG_LINE + 1
    for mode in ("count", "fail"):
        assert kc.count(ok, long_lines=mode) == ([(b"9", 1, 5, 5)], {"lines": 1, "counted": 1, "a_tokens": 0, "long_lines": 0})
    assert kc.count(over)[1]["long_lines"] == 1 and kc.count(over)[0] == [(b"9", 1, 5, 5)]
    with pytest.raises(kc.FormatError) as e:
        kc.count(line(b"9:1") + over, long_lines="fail")
    assert e.value.line == 2
    # NUL bytes do not count towards the line's length
    assert kc.count(over[:5] + b"\0" * 9 + over[5:-2] + b"\n", long_lines="fail")[0] == [(b"9", 1, 0, 0)]


def test_helper_fast_path_equals_the_state_machine():
    rng = np.random.default_rng(2)
    text = random_text(rng, 200000)
    assert kc.count(text) == kc.count(text, fast=False)
    # ... and on bytes thrown into such a text wherever they land, the state machine alone decides
    junk = bytearray(random_text(rng, 20000))
    for p in rng.integers(0, len(junk), 300):
        junk[p] = int(rng.choice(list(b"\t :A9\0x\n")))

    def both(**kw):
        try:
            return kc.count(bytes(junk), **kw)
        except kc.FormatError as e:
            return e.line
    assert both() == both(fast=False)


def _host_count(path, case_only=None, csv=None):
    try:
        rows, tot = host.kraken_count_files([path], only=case_only, csv=csv)
        return rows, (tot["lines"], tot["counted_tokens"], tot["a_tokens"]), tot
    except ga.GsError as e:
        m = re.search(r"line (\d+):", str(e))
        assert m and str(path) in str(e), str(e)
        return ("error", int(m.group(1))), None, None


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_host_exact_path_on_hand_written_cases(case, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    path = str(tmp_path / "in.out")
    csv = str(tmp_path / "res.csv")
    open(path, "wb").write(case.data)
    rows, tot, _ = _host_count(path, case.only, csv)
    assert (rows, tot) == (case.expect, case.totals)
    if isinstance(case.expect, tuple):
        assert not os.path.exists(csv)  # nothing is written where the reference throws
    else:
        assert open(csv, "rb").read() == kc.csv(case.expect)


@pytest.mark.parametrize("container", ["plain", "gz", "bgzf"])
def test_host_exact_path_on_files(container, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    rng = np.random.default_rng(17)
    # odd lines among regular ones, a long line, no final newline
    odd = [line(b"7:5 007:2", cls=b"007"), line(b"9x:5 9:2"), line(b"9:\x005"), line(b"9:5 "), line(b"0:1", cls=b"7", desc=b"d1:5 22:7 z"),
           long_line(LONG_LINE + 5), b"C\td\t9\t9:5\n"]
    parts = []
    for o in odd:
        parts += [random_text(rng, int(rng.integers(3000, 9000))), o]
    data = b"".join(parts) + line(b"9:73")[:-1]
    pack = {"plain": lambda d: d, "gz": gzip.compress, "bgzf": lambda d: bgzf(d, block=4000)}[container]
    path = str(tmp_path / ("in.out" + ("" if container == "plain" else ".gz")))
    open(path, "wb").write(pack(data))
    want_rows, want_tot = kc.count(data)
    for ext in (".csv", ".csv.gz"):
        csv = str(tmp_path / ("res" + ext))
        rows, _, tot = _host_count(path, None, csv)
        assert rows == want_rows
        assert (tot["lines"], tot["counted_tokens"], tot["a_tokens"], tot["long_lines"]) == tuple(want_tot.values())
        assert tot["device_chunks"] == 0
        got = gzip.open(csv).read() if ext.endswith(".gz") else open(csv, "rb").read()
        assert got == kc.csv(want_rows)
    # two files are two streams into one table; an empty line ends its own stream only
    p2 = str(tmp_path / "second.out")
    open(p2, "wb").write(line(b"9:1") + b"\n" + line(b"9:1000"))
    rows, _ = host.kraken_count_files([p2, path, p2], only=[b"9", b"007", b"12345"])
    merged = {}
    for k, *v in kc.count(data)[0] + kc.count(line(b"9:1"))[0] * 2:
        merged[k] = [a + b for a, b in zip(merged.get(k, [0, 0, 0]), v)]
    assert rows == [(k, *merged[k]) for k in sorted(merged) if k in (b"9", b"007")]


def test_write_kraken_csv(tmp_path):
    rows = [(b"", 1, 2, 3), (b"1", 0, 0, 0), (b"10", 5, 1 << 40, 7), (b"2", 1, 1, 1)]
    for name in ("a.csv", "a.csv.gz"):
        p = str(tmp_path / name)
        host.write_kraken_csv(p, rows)
        got = gzip.open(p).read() if name.endswith(".gz") else open(p, "rb").read()
        assert got == kc.csv(rows) == b"taxid;reads;kmers;kmers in matching reads\n;1;2;3;\n1;0;0;0;\n10;5;1099511627776;7;\n2;1;1;1;\n"
    host.write_kraken_csv(str(tmp_path / "e.csv"), [])
    assert open(tmp_path / "e.csv", "rb").read() == b"taxid;reads;kmers;kmers in matching reads\n"


def test_new_calls_without_a_device():
    lib = ga.lib()
    assert lib.gs_krakencount_submit(None, None, 0, 0, None) == -1
    assert lib.gs_krakencount_fetch(None, None, None, 0, None) == -1
    assert lib.gs_krakencount_destroy(None) == 0
    assert ga.abi_version() == 3
    with pytest.raises(ga.GsError):
        host.kraken_count_files(["/nonexistent/kraken.out"])


@pytest.mark.parametrize("write_all", [True, False])
def test_identities_on_the_oracle(write_all):
    """oracle segments + tests/krakenlines.py give the file a match run would write; counted, it must add up to the run's own table"""
    sdb = synth.SynthDB(genera=2, species_per_genus=2, genome_len=4000, seed=5)
    odb = orc.DB(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    recs = sample_reads(sdb.genomes, 400, np.random.default_rng(8))
    seq, off = orc.pack_reads([r for _, r in recs])
    res = matchcheck.oracle_batch(odb, seq, off, max_read_class_err=-1.0)
    text = b"".join(krakenlines.line(d, len(r), 31, odb.segments(r, cap=len(r) + 1) if len(r) >= 31 else [], int(c), sdb.taxids, write_all)
                    for (d, r), c in zip(recs, res["class_vi"]))
    rows, tot = kc.count(text)
    assert kc.count(text, fast=False) == (rows, tot)  # (our own lines are inside the device's grammar)
    assert all(kc.in_grammar(l) for l in text.split(b"\n")[:-1])
    n_class = int((res["class_vi"] >= 0).sum())
    assert 0 < n_class < len(recs) and tot["a_tokens"] > 0 and any(len(r) < 31 for _, r in recs)
    assert tot["lines"] == (sum(len(r) >= 31 for _, r in recs) if write_all else n_class)
    check_identities(rows, res["table"], sdb.taxids)
    assert sum(r[1] for r in rows if r[0] != b"0") == n_class


def test_parser_on_its_own_under_the_address_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=alignment", "-std=c++17", "-Wall"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("no sanitizer runtime")
    exe = str(tmp_path / "krakenparse_sanitize")
    b = subprocess.run(["g++", *flags, "-o", exe, os.path.join(os.path.dirname(__file__), "native", "krakenparse_sanitize.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-800:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
