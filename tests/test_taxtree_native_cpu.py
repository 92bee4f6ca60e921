"""The native host part of the taxtree goals as a stand-alone program under sanitizers: genestrip_amd/csrc/gs_taxparse.h under
AddressSanitizer / UBSan (tests/native/taxparse_sanitize.cpp) on the hand-worked cases of tests/taxtree_cases.py and on generated
dumps, held to tests/taxtree.py.  The program checks on its own that two feeds give what one gives and that select and the small
tree stay inside their arrays."""
import os
import shutil
import subprocess

import pytest

import taxtree
from taxtree_cases import CASES, NAMES_CASES, N, chain_dump, random_dump, star_dump

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
MODE = ["-O1", "-g", "-fsanitize=address,undefined", "-std=c++17"]


def _expected(nodes, names):
    try:
        slots = taxtree.nodes_slots(nodes)
        t = taxtree.Tree(slots)
    except taxtree.Throws as e:
        return ("fails", 1, e.line)
    except taxtree.Unsupported as e:
        return ("fails", 2, e.line)
    try:
        t.read_names(names)
    except taxtree.Throws as e:
        return ("names", 1, e.line)
    rows = [(int(t.taxids[v]), int(t.parent[v]), int(t.depth[v]), int(t.position[v]), int(t.subtree[v]), int(t.rank[v]), t.names[v]) for v in range(t.n)]
    return ("ok", t.n, t.duplicates, len(taxtree.next_lines(nodes)), rows)


def _parse(stdout):
    out, cur = {}, None
    for ln in stdout.splitlines():
        w = ln.split()
        if ln.startswith("case "):
            cur = int(w[1])
            out[cur] = (w[2], int(w[3]), int(w[4])) if w[2] != "ok" else ("ok", int(w[3]), int(w[4]), int(w[5]), [])
        elif ln.startswith("  ") and cur is not None:
            name = None if w[6] == "0" else bytes.fromhex(w[7]) if len(w) > 7 else b""
            out[cur][4].append(tuple(int(x) for x in w[:6]) + (name,))
    return out


def test_parser_and_host_tree_on_the_cases_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "taxparse_sanitize")
    # is the toolchain there?  Decided on a probe of its own, before the code under test is touched
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *MODE, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    b = subprocess.run(["g++", *MODE, "-o", exe, os.path.join(HERE, "taxparse_sanitize.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    cases = [(CASES[n][0], b"") for n in sorted(CASES)] + [(NAMES_CASES[n][0], NAMES_CASES[n][1]) for n in sorted(NAMES_CASES)]
    for nodes in (random_dump(1500, seed=41), chain_dump(3000), star_dump(2000)):
        ids = [s[0] for s in taxtree.nodes_slots(nodes)]
        cases.append((nodes, b"".join(N(t, f"n{t}", "scientific name" if t % 2 else "synonym") for t in ids[::3]) + N(ids[0], "again")))
    # a dump with the oddities of the hand-worked cases between its lines, and without a final newline
    lines = random_dump(600, seed=42).splitlines(keepends=True)
    odd = [b"77\t|\n", b"\n", b"8\x008\t|\t1\t|\tgenus\t|\r\n", lines[3][:-1] + b"x" * 4500 + b"\n", b"99\t|\t1\t|\n"]
    cases.append((b"".join(ln + (odd[(i // 7) % len(odd)] if i % 7 == 0 else b"") for i, ln in enumerate(lines))[:-1], b""))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(f"{len(cases)}\n".encode())
        for nodes, names in cases:
            f.write(f"{len(nodes)}\n".encode() + nodes + b"\n" + f"{len(names)}\n".encode() + names + b"\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fails 0" in r.stdout and "FAILED" not in r.stdout, (r.stdout[-800:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    got = _parse(r.stdout)
    assert len(got) == len(cases)
    kinds = set()
    for i, (nodes, names) in enumerate(cases):
        want = _expected(nodes, names)
        kinds.add(want[0])
        assert got[i] == want, (i, got[i][:4], want[:4])
    assert kinds == {"ok", "fails", "names"}


def test_kernels_on_a_host_stand_in_under_sanitizers(tmp_path):
    """genestrip_amd/csrc/gs_taxtree.hip compiled for the host (tests/native/taxtree_emulate.cpp: a block is 256 real threads) under
    AddressSanitizer / UBSan, every array exactly as large as the library makes it: slots, the arrays of the finish, select, the
    small tree, the names keys and pool, and refusals equal to gs_taxparse.h"""
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
    for name in ("hip/hip_runtime.h", "rocprim/device/device_radix_sort.hpp", "rocprim/device/device_scan.hpp"):  # what gs_taxtree.hip and its headers include
        (tmp_path / "stub" / name).write_text('#include "taxtree_emulate_hip.h"\n')
    exe = str(tmp_path / "taxtree_emulate")
    flags = [*mode, "-x", "c++", "-I", str(tmp_path / "stub"), "-I", HERE]
    b = subprocess.run(["g++", *flags, "-o", exe, os.path.join(HERE, "taxtree_emulate.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count(" ok\n") == 3
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
