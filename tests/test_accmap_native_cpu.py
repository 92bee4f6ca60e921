"""The native parts of the accession map goals as stand-alone programs under sanitizers.  genestrip_amd/csrc/gs_accmapparse.h under AddressSanitizer / UBSan (tests/native/accmapparse_sanitize.cpp):
the hand-worked cases of tests/accmap_cases.py and generated catalogs, held to the expected values and to tests/accmap.py.  The
program checks on its own that two feeds give what one gives and that its index answers every key with its first entry."""
import os
import shutil
import subprocess

import pytest

import accmap
from accmap_cases import CASES, KNOWN, catalog, cfg_of

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
MODE = ["-O1", "-g", "-fsanitize=address,undefined", "-std=c++17"]


def _case_bytes(text, cfg, known):
    dna, rna, mrna = accmap.SEQ_TYPES[cfg["seq_type"]]
    head = [f"{dna} {rna} {mrna}", str(len(cfg["categories"])), *cfg["categories"], str(len(cfg["statuses"])), *cfg["statuses"], str(len(known)),
            " ".join(str(t) for t in known), str(len(text))]
    return ("\n".join(head) + "\n").encode() + text + b"\n"


def _parse(stdout):
    """-> {case: ("throws", line) | ("ok", passing, lines, entries)}"""
    out, cur = {}, None
    for ln in stdout.splitlines():
        w = ln.split()
        if ln.startswith("case "):
            cur = int(w[1])
            out[cur] = ("throws", int(w[3])) if w[2] == "throws" else ("ok", int(w[3]), int(w[4]), [])
        elif ln.startswith("  ") and cur is not None and len(w) <= 2:
            key, node = (b"", w[0]) if len(w) == 1 else (bytes.fromhex(w[0]), w[1])
            out[cur][3].append((key, int(node)))
    return out


def test_parser_on_the_cases_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "accmapparse_sanitize")
    b = subprocess.run(["g++", *MODE, "-o", exe, os.path.join(HERE, "accmapparse_sanitize.cpp")], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    names = sorted(CASES)
    generated = [(catalog(2000, seed=s), dict(cfg_of("plain"), seq_type=t)) for s, t in ((11, "GENOMIC"), (12, "ALL"), (13, "ALL_RNA"))]
    # a generated catalog with the oddities of the hand-worked cases in between its lines: the buffer carries across them
    lines = catalog(400, seed=14).splitlines(keepends=True)
    odd = [CASES[n][0] for n in ("two_tabs_pass_by_overlap", "four_tabs", "three_tabs", "nul_bytes", "one_tab_and_none", "empty_line_in_the_middle")]
    mixed = b"".join(ln + (odd[i % len(odd)].rstrip(b"\0") if i % 7 == 0 else b"") for i, ln in enumerate(lines)) + b"bacteria\tREVIEWED\tNC"
    generated.append((mixed, cfg_of("plain")))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(f"{len(names) + len(generated)}\n".encode())
        for n in names:
            f.write(_case_bytes(CASES[n][0], cfg_of(n), KNOWN))
        for text, cfg in generated:
            f.write(_case_bytes(text, cfg, KNOWN))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fails 0" in r.stdout and "FAILED" not in r.stdout, (r.stdout[-800:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = _parse(r.stdout)
    assert len(got) == len(names) + len(generated)
    for i, n in enumerate(names):
        _, _, passing, entries, n_lines, throws = CASES[n]
        assert got[i] == (("throws", throws) if throws is not None else ("ok", passing, n_lines, entries)), n
    for j, (text, cfg) in enumerate(generated):
        passing, entries, n_lines = accmap.process_catalog(text, cfg["seq_type"], cfg["categories"], cfg["statuses"], KNOWN)
        assert got[len(names) + j] == ("ok", passing, n_lines, entries), j
        assert passing > len(entries) > 20


def test_kernels_on_a_host_stand_in_under_sanitizers(tmp_path):
    """genestrip_amd/csrc/gs_accmap.hip compiled for the host (tests/native/accmap_emulate.cpp: a block is 256 real threads) under
    AddressSanitizer / UBSan, every array exactly as large as the library makes it: counts, entries, order, refusals and lookups
    equal to gs_accmapparse.h"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    # is the toolchain there?  Decided on a probe of its own, before the code under test is touched
    mode = ["-O1", "-g", "-fsanitize=address,undefined", "-std=c++20", "-pthread"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <barrier>\nint main() { std::barrier<> b(1); b.arrive_and_wait(); return 0; }\n")
    if subprocess.run(["g++", *mode, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("no C++20 library with <barrier> or no sanitizer runtime")
    (tmp_path / "stub" / "hip").mkdir(parents=True)
    (tmp_path / "stub" / "rocprim" / "device").mkdir(parents=True)
    (tmp_path / "stub" / "hip" / "hip_runtime.h").write_text('#include "accmap_emulate_hip.h"\n')  # what gs_accmap.hip and gs_launch.h include
    (tmp_path / "stub" / "rocprim" / "device" / "device_radix_sort.hpp").write_text('#include "accmap_emulate_hip.h"\n')
    exe = str(tmp_path / "accmap_emulate")
    flags = [*mode, "-x", "c++", "-I", str(tmp_path / "stub"), "-I", HERE]
    b = subprocess.run(["g++", *flags, "-o", exe, os.path.join(HERE, "accmap_emulate.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count(" ok\n") >= 45
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
