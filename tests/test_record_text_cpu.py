"""Per-read outputs of FASTA and general FASTQ chunks: the text kernels on a host stand-in under sanitizers, and what the new C ABI
calls answer without a device."""
import os
import shutil
import subprocess

import pytest

import genestrip_amd as ga
import streamgoals

GS_E_INVALID = -1


def test_new_calls_refuse_null_without_a_device():
    lib = ga.lib()
    assert lib.gs_match_compact_records(None, 0, 0, None, None, None) == GS_E_INVALID
    assert lib.gs_filter_compact_records(None, 1, 0, 0, None, None, None) == GS_E_INVALID
    assert lib.gs_reads_compact_records(None, 0, 0, None, None, None) == GS_E_INVALID
    assert lib.gs_match_kraken_records(None, 1, 0, None, None, None) == GS_E_INVALID
    assert ga.abi_version() == 3
    for name in ("gs_match_compact_records", "gs_filter_compact_records", "gs_reads_compact_records", "gs_match_kraken_records"):
        assert name in ga.ABI_SYMBOLS


def test_host_stat_3_exists_without_a_device():
    from genestrip_amd import host
    assert host.stat(3) == 0  # (no file has gone through this process)
    assert host.stat(4) == -1


def test_reference_formatter_of_the_gpu_tests_by_hand():
    """streamgoals.read_entries is what the GPU tests build their expectation from: its rule for the shapes they use, by hand"""
    ml = b"@a x\nAC\nGT\n+\nII\nIIJ\n@\nA\n+a\nI\n"
    assert list(streamgoals.read_entries(ml, False)) == [(b"@a x", b"ACGT", b"IIIIJ"), (b"@", b"A", b"I")]
    fa = b">h1\n>h2 d\nAC\r\nG\r\n"
    assert list(streamgoals.read_entries(fa, True)) == [(b"@h1", b"", None), (b"@h2 d", b"AC\rG\r", None)]


def test_record_kernels_on_a_host_stand_in_under_sanitizers(tmp_path):
    """genestrip_amd/csrc/gs_rewrite.hip and the record instantiation of gs_kraken.hip compiled for the host
    (tests/native/records_emulate.cpp: a block is 256 real threads) under AddressSanitizer / UBSan: text equal to a plain formatter's,
    nothing written outside the output"""
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
    (stub / "hip_runtime.h").write_text('#include "records_emulate_hip.h"\n')  # what the .hip files and gs_launch.h include
    exe = str(tmp_path / "records_emulate")
    flags = [*mode, "-x", "c++", "-I", str(tmp_path / "stub"), "-I", here]
    b = subprocess.run(["g++", *flags, "-o", exe, os.path.join(here, "records_emulate.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-800:], r.stderr[-3000:])
    assert r.stdout.count(" ok\n") >= 80
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
