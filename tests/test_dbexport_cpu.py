"""CPU checks of the store export (gs_export.hip): the layout inverses it decodes with (gs_layout.h, built with g++) and the Python
restatement of the reference's db2fastq text that the GPU tests compare against."""
import os
import random
import shutil
import subprocess

import pytest

from fastqgen import fastq_text, kmer_straight, revcomp

HERE = os.path.dirname(os.path.abspath(__file__))


def _harness(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "export_layout_check")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "native", "export_layout_check.cpp")],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe


def test_unmix_inverts_mix(tmp_path):
    r = subprocess.run([_harness(tmp_path), "mix"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fails 0" in r.stdout, r.stdout[-1000:]


def _planes_of(x, k):
    """reference key -> forward planes (bit i = high / low code bit of base i, base 0 = the top bits of x)"""
    hi = lo = 0
    for i in range(k):
        c = (x >> (2 * (k - 1 - i))) & 3
        hi |= (c >> 1) << i
        lo |= (c & 1) << i
    return hi, lo


def _palindrome(k, rng):
    half = [rng.randrange(4) for _ in range(k // 2)]
    codes = half + [c ^ 1 for c in reversed(half)]
    x = 0
    for c in codes:
        x = (x << 2) | c
    return x


def test_planes_to_reference_key(tmp_path):
    """gs_planes_to_kmer: planes of EITHER strand -> max(fwd, revcomp) of the interleaved encoding (CGAT.java:145-147)"""
    rng = random.Random(7)
    cases = []
    for k in (15, 16, 17, 19, 21, 22, 25, 30, 31):
        xs = [rng.randrange(4 ** k) for _ in range(300)] + [0, 4 ** k - 1]
        if k % 2 == 0:
            xs += [_palindrome(k, rng) for _ in range(50)]
        for x in xs:
            for y in (x, revcomp(x, k)):  # both orientations must give the same key
                cases.append((k, y, max(x, revcomp(x, k))))
    inp = "".join("%d %d %d\n" % (k, *_planes_of(y, k)) for k, y, _ in cases)
    r = subprocess.run([_harness(tmp_path), "keys"], input=inp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1000:]
    got = [int(t) for t in r.stdout.split()]
    assert len(got) == len(cases)
    bad = [(c, g) for c, g in zip(cases, got) if g != c[2]]
    assert not bad, bad[:5]
    assert any(x == revcomp(x, k) for k, x, _ in cases if k % 2 == 0)  # palindromes were in the set


def test_fastq_restatement_by_hand():
    """FastQWriter's bytes for two k-mers: the "::" of GENESTRIP_ID + ":" + (project + ":") + ':' + taxid, reads from 1"""
    k = 4
    kmers = [0b00011011, 0b11111111]  # C G A T, T T T T
    assert kmer_straight(kmers[0], k) == "CGAT"
    got = fastq_text(kmers, [1, 0], ["9606", "562"], k, "human_virus")
    assert got == (b"@GENESTRIP:human_virus::562:1\nCGAT\n+\n~~~~\n"
                   b"@GENESTRIP:human_virus::9606:2\nTTTT\n+\n~~~~\n")
