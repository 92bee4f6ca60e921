"""The per-record arithmetic of gs_sn_reduce_kernel (gs_sn_row, genestrip_amd/csrc/gs_snrec.h) in a stand-alone program under
AddressSanitizer / UBSan (tests/native/snrec_steps.cpp; nothing here is loaded into python): contigs, sum of squared lengths, longest
contig, class, flags and the row of a record against a position-by-position walk, for all 2^16 masks on positions 56 .. 71, every
single-run mask and seeded random masks at max = 98, 120 and 128 positions, under ten settings of classification, threshold and error
gates."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("snrec_steps")
    mode = ["-O1", "-g", "-fsanitize=address,undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *mode, "-std=c++17", "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("no sanitizer runtime")
    out = str(tmp / "snrec_steps")
    b = subprocess.run(["g++", *mode, "-std=c++17", "-o", out, os.path.join(HERE, "snrec_steps.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


def test_record_row_equals_the_position_walk(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    # 3 lengths x 10 settings x (2 x 65535 masks at the boundary + every single run + 4000 random masks)
    assert int(r.stdout.split("checked ")[1].split()[0]) > 3 * 10 * (2 * 65535 + 98 * 99 // 2 + 4000)
