"""The regions kernels of genestrip_amd/csrc/gs_taxtree.hip compiled for the host (tests/native/regions_emulate.cpp: a block is 256
real threads) as a stand-alone program under AddressSanitizer / UBSan, every array exactly as large as gs_taxtree_regions_below makes
it, on trees whose node counts lie around a wave and a block, held to the parent walk of gs_taxparse.h."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_regions_kernels_on_a_host_stand_in_under_sanitizers(tmp_path):
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
    exe = str(tmp_path / "regions_emulate")
    flags = [*mode, "-x", "c++", "-I", str(tmp_path / "stub"), "-I", HERE]
    b = subprocess.run(["g++", *flags, "-o", exe, os.path.join(HERE, "regions_emulate.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count(" ok\n") == 6
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
