"""The host-checkable halves of gs_pf_kernel (genestrip_amd/csrc/gs_prefilter.h) in a stand-alone program under AddressSanitizer /
UBSan (tests/native/prefilter_steps.cpp; nothing here is loaded into python):
(i) the grouped decision equals gs_pf_read_passes read for read, is decided by the first sample gs_pf_sample_in accepts, never asks
the exact level where level one is clear and never twice for a sample -- over the reads of tests/test_prefilter_cpu.py (both
strands, substitutions, N, lower case, CR) at m = 5 .. 27 samples and over constructed reads in which a chosen sample decides,
with decoys (level one set, not in S) in front of it;
(ii) the copy's index arithmetic, exhaustively over base alignment, reads per round and L = 32 .. 158."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from genestrip_amd import synth
import prefilter as pf
import prefilter_cases as pc
from prefilter import make_reads

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
CASES = [(31, 128), (31, 150), (31, 158), (31, 95), (25, 128), (25, 150), (25, 152), (19, 83), (19, 146)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("prefilter_steps")
    mode = ["-O1", "-g", "-fsanitize=address,undefined"]
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *mode, "-std=c++17", "-o", str(tmp / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("no sanitizer runtime")
    out = str(tmp / "prefilter_steps")
    b = subprocess.run(["g++", *mode, "-std=c++17", "-o", out, os.path.join(HERE, "prefilter_steps.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def sets():
    out = {}
    for k in (31, 25, 19):
        db = synth.SynthDB(k=k, genera=2, species_per_genus=3, genome_len=20000, seed=3)
        out[k] = (db, pf.lmer_set(db.kmers, k))
    return out


def _write_case(path, S, seq, L, k):
    canon, bad = pf.sample_codes(seq, L, k)
    ok = pf.passes(S, seq, L, k)
    with open(path, "wb") as f:
        f.write(struct.pack("<iiiiq", k, L, len(seq), canon.shape[1], len(S)))
        f.write(S.astype("<i8").tobytes())
        f.write(np.ascontiguousarray(seq).tobytes())
        f.write(np.ascontiguousarray(canon).astype("<i8").tobytes())
        f.write(np.ascontiguousarray(bad).astype(np.uint8).tobytes())
        f.write(ok.astype(np.uint8).tobytes())
    return ok


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fails 0" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("k,L", CASES)
def test_grouped_decision_equals_the_sample_walk(exe, sets, tmp_path, k, L):
    db, S = sets[k]
    seq = make_reads(db.genomes, L, k, 1500, seed=100 * k + L)
    ok = _write_case(tmp_path / "case.bin", S, seq, L, k)
    assert 0 < ok.sum() < len(ok)
    assert "case ok" in _run(exe, "decide", str(tmp_path / "case.bin"))


def test_every_sample_decides_and_decoys_are_asked_once(exe, sets, tmp_path):
    _, S = sets[31]
    reads, expect, decider, planted = pc.deciding_sample_reads(S, 150, 31, seed=5)
    assert sorted(set(decider[decider >= 0])) == list(range(8))
    # the reads with an N in the planted sample are a case of their own: the code of such a sample is arbitrary, so whether the
    # exact level is asked for it is not known here; they must be rejected
    _write_case(tmp_path / "with_n.bin", S, reads[~expect], 150, 31)
    out = _run(exe, "decide", str(tmp_path / "with_n.bin"))
    assert "case ok" in out and ", 0 pass," in out.splitlines()[0]
    _write_case(tmp_path / "case.bin", S, reads[expect], 150, 31)
    out = _run(exe, "decide", str(tmp_path / "case.bin"))
    assert "case ok" in out
    line = out.splitlines()[0]  # "... exact level asked A times, B of them not in S ..."
    asked, not_in_s = int(line.split("asked ")[1].split()[0]), int(line.split("times, ")[1].split()[0])
    # the exact level is asked once for every decoy in front of a planted sample and says no, and once for every planted sample;
    # no other sample of these reads passes level one
    assert planted.sum() >= 0 + 1 + 2 * 6 and not_in_s == planted.sum() and asked == planted.sum() + 2 * 8
    assert out.splitlines()[1].split(":")[1].split() == ["2"] * 8  # every sample index decides two reads


def test_copy_index_arithmetic(exe):
    assert "copy ok" in _run(exe, "copy")
