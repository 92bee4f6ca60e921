"""What one lane of gs_sn_walk_kernel does for a read that left the match kernel as its row of node codes (gs_sn_walk,
genestrip_amd/csrc/gs_snrec.h) in a stand-alone program under AddressSanitizer / UBSan (tests/native/snwalk_steps.cpp; nothing here is
loaded into python): every counter, class and flags of a read against a restatement of the reference's matchRead that keeps vote
counts per node and walks parent links, at 98, 120 and 128 positions, 1 .. 8 distinct nodes (ancestor chains, siblings, unrelated,
random), max_paths 1, 2 and 64, thresholds 1 and 3, error gates off and on, non-CGAT bytes in the first, a middle and the last
window and alone, and rows of nothing but MISS and INVALID, on trees of 5 and 25 nodes."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("snwalk_steps")
    mode = ["-O1", "-g", "-fsanitize=address,undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *mode, "-std=c++17", "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("no sanitizer runtime")
    out = str(tmp / "snwalk_steps")
    b = subprocess.run(["g++", *mode, "-std=c++17", "-o", out, os.path.join(HERE, "snwalk_steps.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


def test_walk_equals_the_restated_match_read(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    # 2 trees x 3 lengths x 19 settings x (4 relations x 8 node counts x 12 rows x 8 byte patterns, less the node sets a tree lacks)
    checked, classified = (int(r.stdout.split(w)[1].split()[0]) for w in ("checked ", "reads ("))
    assert checked > 2 * 3 * 19 * 2000 and classified > checked // 4
