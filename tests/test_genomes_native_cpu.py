"""The host side of the genomes stage under AddressSanitizer / UBSan, as stand-alone programs (nothing here is loaded into python):
  * genestrip_amd/csrc/gs_genomeparse.h, the line-by-line parser that takes the chunks the device refuses
    (tests/native/genomeparse_sanitize.cpp: the hand-written streams of tests/genomefasta_cases.py and walks in chunks);
  * the kernels of genestrip_amd/csrc/gs_genomes.hip compiled for the host, a block being 256 real threads
    (tests/native/genomes_emulate.cpp): every array as large as the C ABI makes it, the results those of the parser."""
import os
import re
import shutil
import subprocess

import pytest

from genomefasta_cases import CASES

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
MODE = ["-O1", "-g", "-fsanitize=address,undefined"]


def _clean(r, at_least):
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-800:], r.stderr[-3000:])
    assert r.stdout.count(" ok\n") >= at_least
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def _toolchain(tmp_path, std, body, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text(body)
    if subprocess.run(["g++", *MODE, std, *extra, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("no sanitizer runtime or C++ library for this probe")


def test_host_parser_under_sanitizers(tmp_path):
    _toolchain(tmp_path, "-std=c++17", "int main() { return 0; }\n")
    src = os.path.join(HERE, "genomeparse_sanitize.cpp")
    # the program carries the hand-written streams of the Python cases: by name, all of them
    names = set(re.findall(r'^\s*\{"([^"]+)", ', open(src).read(), re.M))
    assert {c[0] for c in CASES} <= names, {c[0] for c in CASES} - names
    exe = str(tmp_path / "genomeparse_sanitize")
    b = subprocess.run(["g++", *MODE, "-std=c++17", "-o", exe, src], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    _clean(subprocess.run([exe], capture_output=True, text=True, timeout=300), len(CASES) + 100)


def test_genome_kernels_on_a_host_stand_in_under_sanitizers(tmp_path):
    _toolchain(tmp_path, "-std=c++20", "#include <barrier>\nint main() { std::barrier<> b(1); b.arrive_and_wait(); return 0; }\n", ["-pthread"])
    stub = tmp_path / "stub" / "hip"
    stub.mkdir(parents=True)
    (stub / "hip_runtime.h").write_text('#include "genomes_emulate_hip.h"\n')  # what the .hip files and gs_launch.h include
    exe = str(tmp_path / "genomes_emulate")
    flags = [*MODE, "-std=c++20", "-pthread", "-x", "c++", "-I", str(tmp_path / "stub"), "-I", HERE]
    b = subprocess.run(["g++", *flags, "-o", exe, os.path.join(HERE, "genomes_emulate.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    _clean(subprocess.run([exe], capture_output=True, text=True, timeout=900), 140)
