"""The plain-Python restatement of the Kraken-style line (tests/krakenlines.py) against the golden KrakenUniq line, its descriptor
rule by hand, and what the new C ABI calls answer without a device."""
import os

import numpy as np
import pytest

import genestrip_amd as ga
import krakenlines
from conftest import GOLDEN
from oracle import gs_oracle as orc

GS_E_INVALID = -1


def test_helper_reproduces_the_golden_dengue_line():
    lines = open(os.path.join(GOLDEN, "dengue1", "dengue1.fasta")).read().split("\n")
    genome = "".join(l.strip() for l in lines if not l.startswith(">")).upper()
    keys = np.unique(orc.canonical_kmers(genome, 31))
    odb = orc.DB(31, keys, np.zeros(len(keys), np.int32), 1, np.array([-1], np.int32))
    text = open(os.path.join(GOLDEN, "dengue1", "test.fastq"), "rb").read()
    rd = orc.parse_fastq(text, k=31)
    run = orc.MatchRun(odb, classify=True)
    cv, _ = run.submit(rd["seq"], rd["seq_off"])
    run.close()
    got = krakenlines.chunk_lines(text, 31, odb.segments, cv, ["1"])
    golden = open(os.path.join(GOLDEN, "dengue1", "test.out"), "rb").read()
    assert b"".join(got) == golden == b"C\ttest\t1\t41\t0:2 1:7 0:2\n"
    # not classified: 'U' and taxid 0 with write_all, nothing without
    assert b"".join(krakenlines.chunk_lines(text, 31, odb.segments, [-1], ["1"])) == b"U\ttest\t0\t41\t0:2 1:7 0:2\n"
    assert krakenlines.chunk_lines(text, 31, odb.segments, [-1], ["1"], write_all=False) == [b""]


def test_descriptor_rule_by_hand():
    assert krakenlines.name_of(b"@") == b""
    assert krakenlines.name_of(b"") == b""
    assert krakenlines.name_of(b"@ x") == b""           # the blank at index 1 ends an empty name
    assert krakenlines.name_of(b"@name ") == b"name"    # a blank at the end
    assert krakenlines.name_of(b"@name") == b"name"     # no blank
    assert krakenlines.name_of(b"@a b c") == b"a"
    assert krakenlines.name_of(b" a b") == b"a"         # the first byte is dropped whatever it is, a blank too
    assert krakenlines.name_of(b"@na\tme\r") == b"na\tme\r"  # TAB and '\r' are bytes like any other
    assert krakenlines.name_of(b"@n\xc3\xa4me x") == b"n\xc3\xa4me"


def test_line_by_hand():
    tax = ["10", "", "1234567"]
    assert krakenlines.line(b"@r1 d", 5, 2, [(0, 1), (-1, 2), (-2, 1)], 0, tax) == b"C\tr1\t10\t5\t10:1 0:2 A:1\n"
    assert krakenlines.line(b"@r1", 5, 2, [(1, 4)], 1, tax) == b"C\tr1\t\t5\t:4\n"  # an empty taxid string
    assert krakenlines.line(b"@r1", 5, 2, [(2, 4)], -1, tax, write_all=True) == b"U\tr1\t0\t5\t1234567:4\n"
    assert krakenlines.line(b"@r1", 5, 2, [(2, 4)], -1, tax, write_all=False) == b""
    assert krakenlines.line(b"@r1", 1, 2, [], 0, tax) == b""  # no position: no line
    # CRLF: the '\r' belongs to the descriptor and to the read (counted into L)
    recs = krakenlines.records(b"@r1\r\nACGT\r\n+\r\nIIII\r\n@r2 x\r\nAC\r\n+\r\nII\r\n")
    assert recs == [(b"@r1\r", b"ACGT\r"), (b"@r2 x\r", b"AC\r")]


def test_new_calls_refuse_null_without_a_device():
    lib = ga.lib()
    assert lib.gs_match_set_taxids(None, None) == GS_E_INVALID
    assert lib.gs_match_kraken_text(None, 1, 0, None, None, None) == GS_E_INVALID
    assert lib.gs_match_kraken_time(None, None, None) == GS_E_INVALID
    assert ga.abi_version() == 3


def test_text_kernels_on_a_host_stand_in_under_sanitizers(tmp_path):
    """genestrip_amd/csrc/gs_kraken.hip compiled for the host (tests/native/kraken_emulate.cpp: a block is 256 real threads) under
    AddressSanitizer / UBSan: text equal to a straightforward formatter's, nothing written outside the output"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    # is the toolchain there?  Decided on a probe of its own, before the code under test is touched: whatever goes wrong with the
    # build of the kernels afterwards fails the test
    mode = ["-O1", "-g", "-fsanitize=address,undefined", "-std=c++20", "-pthread"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <barrier>\nint main() { std::barrier<> b(1); b.arrive_and_wait(); return 0; }\n")
    if subprocess.run(["g++", *mode, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("no C++20 library with <barrier> or no sanitizer runtime")
    here = os.path.join(os.path.dirname(__file__), "native")
    stub = tmp_path / "stub" / "hip"
    stub.mkdir(parents=True)
    (stub / "hip_runtime.h").write_text('#include "kraken_emulate_hip.h"\n')  # what gs_kraken.hip and gs_launch.h include
    exe = str(tmp_path / "kraken_emulate")
    flags = [*mode, "-x", "c++", "-I", str(tmp_path / "stub"), "-I", here]
    b = subprocess.run(["g++", *flags, "-o", exe, os.path.join(here, "kraken_emulate.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-800:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
