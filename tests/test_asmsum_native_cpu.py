"""The native parts of the fastasgenbank goal as stand-alone programs under sanitizers.  genestrip_amd/csrc/gs_asmsumparse.h under
AddressSanitizer / UBSan (tests/native/asmsumparse_sanitize.cpp): the hand-worked cases of tests/asmsum_cases.py and generated
summaries, held to the expected values and to tests/asmsum.py.  The program checks on its own that two feeds cut at any byte give
what one feed gives.  The kernels of gs_asmsum.hip compiled for the host (tests/native/asmsum_emulate.cpp) are held to the parser."""
import os
import shutil
import subprocess

import pytest

import asmsum
from asmsum_cases import CASES, KNOWN, cfg_of

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
MODE = ["-O1", "-g", "-fsanitize=address,undefined", "-std=c++17"]


def _case_bytes(text, c, max_per_node):
    flt = [] if c["filter"] is None else [int(i in c["filter"]) for i in range(len(c["known"]))]
    head = [f"{c['quality_mask']} {int(c['reference_only'])} {int(c['use_species_taxid'])} {max_per_node}", str(len(c["known"])),
            " ".join(str(t) for t in c["known"]), str(len(flt)), " ".join(str(x) for x in flt), str(len(text))]
    return ("\n".join(head) + "\n").encode() + text + b"\n"


def _unhex(w):
    return b"" if w == "-" else bytes.fromhex(w)


def _parse(stdout):
    """-> {case: ("throws", line) | ("ok", counted, short, skipped, lines, entries, picked entry numbers, nodes with entries)}"""
    out, cur = {}, None
    for ln in stdout.splitlines():
        w = ln.split()
        if ln.startswith("case "):
            cur = int(w[1])
            out[cur] = ["throws", int(w[3])] if w[2] == "throws" else ["ok", int(w[3]), int(w[4]), int(w[5]), int(w[6]), [], [], int(w[9])]
        elif ln.startswith("  e ") and cur is not None:
            out[cur][5].append((int(w[1]), _unhex(w[5]), _unhex(w[6]), _unhex(w[7]), int(w[2]), bool(int(w[3])), int(w[4])))
        elif ln.startswith("  p") and cur is not None:
            out[cur][6] = [int(x) for x in w[1:]]
    return out


def test_parser_on_the_cases_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    # is the toolchain there?  Decided on a probe of its own, before the code under test is touched
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <string>\nint main() { std::string s(3, 'x'); return (int)s.size() - 3; }\n")
    if subprocess.run(["g++", *MODE, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    exe = str(tmp_path / "asmsumparse_sanitize")
    b = subprocess.run(["g++", *MODE, "-o", exe, os.path.join(HERE, "asmsumparse_sanitize.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    names = sorted(CASES)
    known = sorted(set(KNOWN) | {1000 + 13 * i for i in range(40)})
    generated = []
    for seed, kw, max_per_node in ((11, {}, 1), (12, {"quality_mask": -1, "use_species_taxid": True}, 2),
                                   (13, {"quality_mask": 0x7fe, "reference_only": True, "filter": set(range(0, len(known), 2))}, 1)):
        text = asmsum.summary(1200, known, seed=seed)
        lines = text.split(b"\n")
        # the oddities of the hand-worked cases in between its lines: CR LF, lone CRs, a U+0131 key, NUL bytes
        text = b"".join(ln + (b"\r\n" if i % 5 == 0 else b"\r" if i % 17 == 0 else b"\n") for i, ln in enumerate(lines[:-1]))
        text += CASES["high_byte_in_the_key"][0] + CASES["nul_bytes_are_data"][0] + CASES["unterminated_last_line"][0]
        generated.append((text, asmsum.cfg(known, **kw), max_per_node))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(f"{len(names) + len(generated)}\n".encode())
        for n in names:
            f.write(_case_bytes(CASES[n][0], cfg_of(n), 0))
        for text, c, max_per_node in generated:
            f.write(_case_bytes(text, c, max_per_node))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fails 0" in r.stdout and "FAILED" not in r.stdout, (r.stdout[-800:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = _parse(r.stdout)
    assert len(got) == len(names) + len(generated)
    for i, n in enumerate(names):
        _, _, entries, counted, short, skipped, throws, _ = CASES[n]
        if throws is not None:
            assert got[i] == ["throws", throws], n
        else:
            assert got[i][:6] == ["ok", counted, short, skipped, counted + short + skipped, entries], n
            assert [entries[j] for j in got[i][6]] == asmsum.cap(entries, 0), n
    for j, (text, c, max_per_node) in enumerate(generated):
        entries, counted, short, skipped = asmsum.relevant_entries(text, c)
        g = got[len(names) + j]
        assert g[:6] == ["ok", counted, short, skipped, counted + short + skipped, entries], j
        want = asmsum.cap(entries, max_per_node)
        assert [entries[i] for i in g[6]] == want and g[7] == len({e[0] for e in entries}), j
        assert counted > len(entries) > 40 and len(entries) - len(want) > 5


def test_kernels_on_a_host_stand_in_under_sanitizers(tmp_path):
    """genestrip_amd/csrc/gs_asmsum.hip compiled for the host (tests/native/asmsum_emulate.cpp: a block is 256 real threads) under
    AddressSanitizer / UBSan, every array exactly as large as the library makes it: counts, entries with their strings and lines,
    refusals with their first bad line, and the cap equal to gs_asmsumparse.h"""
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
    (tmp_path / "stub" / "hip" / "hip_runtime.h").write_text('#include "asmsum_emulate_hip.h"\n')  # what gs_asmsum.hip and gs_launch.h include
    for name in ("device_radix_sort.hpp", "device_scan.hpp"):
        (tmp_path / "stub" / "rocprim" / "device" / name).write_text('#include "asmsum_emulate_hip.h"\n')
    exe = str(tmp_path / "asmsum_emulate")
    flags = [*mode, "-x", "c++", "-I", str(tmp_path / "stub"), "-I", HERE]
    b = subprocess.run(["g++", *flags, "-o", exe, os.path.join(HERE, "asmsum_emulate.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count(" ok\n") >= 50
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
