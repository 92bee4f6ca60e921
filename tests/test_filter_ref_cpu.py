"""CPU checks behind tests/test_gpu_filter_edges.py: the magic-number division the filter kernel compiles (gs_absmod.h, built
with g++), the oracle's raw-geometry filters and the host references (tests/bloomref.py) against orc.Bloom / filter_batch, and
the fpp -> n_hashes table the GPU cells rely on."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bloomref as br
from oracle import gs_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
# the hash counts of test_gpu_filter_edges.py's staging cells (one row of gs_filter_kernel's staging table or more each)
HASHES = (1, 2, 3, 4, 5, 6, 7, 8, 11, 14, 15, 16, 17, 40, 64)
STAGING_N = 2000  # expected insertions of those cells


def test_magic_division_matches_java_absmod(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "absmod_check")
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "native", "absmod_check.cpp")],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " fails 0" in r.stdout, r.stdout[-2000:]
    assert int(r.stdout.split()[1]) > 2_000_000  # every divisor class and dividend edge ran


@pytest.mark.parametrize("h", HASHES)
def test_fpp_gives_hash_count(h):
    """the staging cells ask for h hashes through fpp = 2^-h; the oracle, gs_bloom_build's formula and bloomref agree"""
    fpp = br.fpp_for_hashes(h)
    for kind in (orc.BLOOM_XOR, orc.BLOOM_MURMUR):
        ob = orc.Bloom(kind, STAGING_N, fpp)
        assert ob.hashes == h
        assert br.geometry(STAGING_N, fpp) == (ob.bits, ob.hashes)
    assert br.geometry(10**9, 0.5)[1] == 1 and br.geometry(5, 0.01)[1] == 7  # the large cell; fpp 0.01


def _random_reads(rng, n, k, alphabet=b"ACGTACGTACGTNa"):
    reads = []
    for _ in range(n):
        L = int(rng.integers(0, 200))
        reads.append(bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), L)))
    return orc.pack_reads(reads) + (reads,)


@pytest.mark.parametrize("kind", [orc.BLOOM_XOR, orc.BLOOM_MURMUR, orc.BLOOM_BLOCKED])
def test_references_match_oracle(kind):
    rng = np.random.default_rng(5 + kind)
    for k, n, fpp in ((31, 300, 0.05), (7, 40, 0.3), (16, 100, 1e-3)):
        ref = orc.Bloom(kind, n, fpp)
        genome = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n + k - 1))
        keys = orc.canonical_kmers(genome, k)
        ref.put_many(keys)
        factors = ref.hash_factors
        bits, nh = ref.bits, max(ref.hashes, 1)
        # the raw constructor with the same geometry is the same filter
        raw = orc.Bloom.raw(kind, bits, nh, factors)
        raw.put_many(keys)
        assert np.array_equal(raw.words, ref.words)
        # and with initial words it starts from them
        assert np.array_equal(orc.Bloom.raw(kind, bits, nh, factors, ref.words).words, ref.words)
        sp = br.SparseBloom(kind, bits, factors)
        for key in keys.tolist():
            sp.put(key)
        dense = np.zeros_like(ref.words)
        for w, v in sp.words.items():
            dense[w] = v
        assert np.array_equal(dense, ref.words)
        pool = np.concatenate([keys, rng.integers(0, 1 << 62, 3000, dtype=np.int64)])
        want = np.array([ref.contains(x) for x in pool.tolist()])
        if kind == orc.BLOOM_BLOCKED:
            got = br.blocked_contains(factors[0], bits, ref.words, pool)
        else:
            got = br.hash_bits(kind, factors, bits, ref.words, pool).all(axis=1)
        assert np.array_equal(got, want)
        assert np.array_equal(np.array([sp.contains(x) for x in pool.tolist()]), want)
        assert want[:len(keys)].all() and not want[len(keys):].all()
        seq, off, reads = _random_reads(rng, 300, k)
        reads += [genome[i:i + int(rng.integers(k, 3 * k))] for i in range(0, n, 7)]
        seq, off = orc.pack_reads(reads)
        for min_pos, ratio in ((1, 0.2), (0, 0.5), (3, 0.0), (0, 0.0)):
            w = ref.filter_batch(k, min_pos, ratio, seq, off)
            assert np.array_equal(raw.filter_batch(k, min_pos, ratio, seq, off), w)
            assert np.array_equal(np.array([sp.accept(r, k, min_pos, ratio) for r in reads], dtype=np.uint8), w)
            assert 0 < w.sum() < len(w)
            if kind != orc.BLOOM_BLOCKED:
                # the staging trace counts members the same way (early exit included)
                for r, a in zip(reads, w):
                    kk, valid = br.read_keys(r, k)
                    if len(kk):
                        hb = br.hash_bits(kind, factors, bits, ref.words, kk)
                        need = br.need_of(len(kk), min_pos, ratio)
                        assert (br.stage_trace(hb, valid, need)["members"] >= need) == bool(a)


def test_raw_geometry_edges():
    """bits = 1 (every key hits bit 0; the kernel's magic shift is 0), 65 and a 1-bucket blocked filter"""
    ob = orc.Bloom.raw(orc.BLOOM_XOR, 1, 3, [1, 2, 3])
    assert ob.bits == 1 and ob.hashes == 3 and len(ob.words) == 1
    assert not ob.contains(12345)
    ob.put(7)
    assert ob.contains(12345) and ob.words[0] == 1
    ob = orc.Bloom.raw(orc.BLOOM_BLOCKED, 1, 0, [99])
    assert len(ob.words) == 18
    with pytest.raises(ValueError):
        orc.Bloom.raw(orc.BLOOM_XOR, 0, 1, [1])
    with pytest.raises(ValueError):
        orc.Bloom.raw(orc.BLOOM_MURMUR, 10, 0, [1])
    # INT64_MIN and +-(2^63 - 1): Java's Math.abs(v % bits), as jabs_mod and SparseBloom compute it
    for bits in (1, 2, 3, 65, 1000003, (1 << 37) - 25):
        for v in (-(1 << 63), (1 << 63) - 1, -(1 << 63) + 1):
            want = abs(v) % bits
            assert int(br.jabs_mod(np.array([v]), bits)[0]) == want
            f = v ^ 12345
            assert br.SparseBloom(orc.BLOOM_XOR, bits, [f]).positions(12345) == [want]
