"""The sampled 15-mer prefilter on the CPU: the restatement (tests/prefilter.py) held to the oracle -- every read in which the oracle
finds a stored k-mer passes -- and the native conversion and probe (genestrip_amd/csrc/gs_prefilter.h) held to the restatement in a
stand-alone program under AddressSanitizer / UBSan (tests/native/prefilter_emulate.cpp; nothing here is loaded into python).
k = 31 and k = 25 (w = 11); L = 128, 150 and k + 127; both strands, substitutions, N, lower case and CR bytes; a read whose only
clean k-mer starts at 0 and one whose only clean k-mer starts at L - k."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from genestrip_amd import synth
from oracle import gs_oracle as orc
import prefilter as pf
from prefilter import make_reads

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
CASES = [(31, 128), (31, 150), (31, 158), (25, 128), (25, 150), (25, 152)]


@pytest.fixture(scope="module")
def stores():
    out = {}
    for k in (31, 25):
        db = synth.SynthDB(k=k, genera=2, species_per_genus=3, genome_len=20000, seed=3)
        out[k] = (db, orc.DB(k, db.kmers, db.value_idx, db.n_values, db.parent_vi), pf.lmer_set(db.kmers, k))
    return out


@pytest.fixture(scope="module")
def batches(stores):
    out = {}
    for k, L in CASES:
        db, odb, S = stores[k]
        n = 1500
        seq = make_reads(db.genomes, L, k, n, seed=100 * k + L)
        run = orc.MatchRun(odb)
        try:
            _, fl = run.submit(seq.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
        finally:
            run.close()
        out[(k, L)] = (seq, (np.asarray(fl) & orc.F_FOUND) != 0)
    return out


def test_sample_positions():
    assert pf.sample_positions(150, 31) == [17 * i for i in range(8)]
    for k in range(19, 32):
        for L in range(128, k + 128):
            pos = pf.sample_positions(L, k)
            w = pf.stride(k)
            assert pos[0] == 0 and pos[-1] + w > L - 15 >= pos[-1] and all(b - a == w for a, b in zip(pos, pos[1:]))
            for s in range(L - k + 1):  # every k-mer owns exactly one sample
                assert sum(s <= p <= s + w - 1 for p in pos) == 1


@pytest.mark.parametrize("k,L", CASES)
def test_no_read_with_a_hit_is_rejected(stores, batches, k, L):
    _, _, S = stores[k]
    seq, found = batches[(k, L)]
    ok = pf.passes(S, seq, L, k)
    assert found[0] and found[1], "the two edge reads must hit in the oracle"
    assert ok[0] and ok[1]
    assert not np.any(found & ~ok), np.flatnonzero(found & ~ok)[:10]
    assert found.sum() > len(found) // 2
    bg = np.arange(len(found)) % 4 == 3
    assert (~ok[bg]).mean() > 0.9  # the filter of a small store rejects nearly all of the background


def test_native_conversion_and_probe_under_sanitizers(stores, batches, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    mode = ["-O1", "-g", "-fsanitize=address,undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *mode, "-std=c++17", "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True).returncode != 0:
        pytest.skip("no sanitizer runtime")
    exe = str(tmp_path / "prefilter_emulate")
    b = subprocess.run(["g++", *mode, "-std=c++17", "-o", exe, os.path.join(HERE, "prefilter_emulate.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    for k, L in CASES:
        _, _, S = stores[k]
        seq, _ = batches[(k, L)]
        canon, bad = pf.sample_codes(seq, L, k)
        ok = pf.passes(S, seq, L, k)
        path = tmp_path / f"case_{k}_{L}.bin"
        with open(path, "wb") as f:
            f.write(struct.pack("<iiiiq", k, L, len(seq), canon.shape[1], len(S)))
            f.write(S.astype("<i8").tobytes())
            f.write(np.ascontiguousarray(seq).tobytes())
            f.write(np.ascontiguousarray(canon).astype("<i8").tobytes())
            f.write(np.ascontiguousarray(bad).astype(np.uint8).tobytes())
            f.write(ok.astype(np.uint8).tobytes())
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "fails 0" in r.stdout and "case ok" in r.stdout and "MISMATCH" not in r.stdout, (r.stdout[-800:], r.stderr[-3000:])
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
