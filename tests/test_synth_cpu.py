"""The synthetic-input builders (genestrip_amd/synth.py, libgssynth.so) against the oracle's restatement: the index
filter a bench / test workload is given must be the one BloomIndexGoal would have built.  CPU only."""
import numpy as np
import pytest

from genestrip_amd import synth
from oracle import gs_oracle as orc


def test_java_random_longs_are_the_reference_hash_factors():
    assert synth.java_random_longs(42, 3).tolist() == [-5025562857975149833, -5843495416241995736, 5694868678511409995]


@pytest.mark.parametrize("n,fpp", [(1000, 1e-8), (50_000, 1e-8), (47_038_401, 1e-8), (20_000, 0.05), (7, 0.5)])
def test_xor_bloom_geometry_equals_the_oracle(n, fpp):
    ob = orc.Bloom(orc.BLOOM_XOR, n, fpp)
    bits, hashes, factors = synth.xor_bloom_geometry(n, fpp)
    assert (bits, hashes) == (ob.bits, ob.hashes)
    assert np.array_equal(factors, ob.hash_factors)
    if fpp == 1e-8:
        assert hashes == 27


def test_xor_bloom_words_equal_the_oracle():
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 1 << 62, 30_000, dtype=np.int64)
    ob = orc.Bloom(orc.BLOOM_XOR, len(keys), 1e-8)
    ob.put_many(keys)
    bits, hashes, factors = synth.xor_bloom_geometry(len(keys), 1e-8)
    words = synth.xor_bloom_host(keys, bits, factors)
    assert np.array_equal(words, ob.words)


# ------------------------------------------------------------------ skewed workloads (synth.SkewedDB, synth.skewed_reads)
@pytest.fixture(scope="module")
def skew():
    return synth.SkewedDB(genera=3, species_per_genus=3, genome_len=60_000, strains=2, dominant_len=2000, n_values=90, seed=4)


def test_skewed_genomes_have_the_promised_shape(skew):
    db = skew
    assert db.n_values == 90 and len(db.parent_vi) == 90 and db.dominant_vi == 89
    assert np.all(db.parent_vi[1:] < np.arange(1, 90)) and db.parent_vi[0] == -1
    for i, vi in enumerate(db.species_vi[:-len(db.strain_vi)]):
        g = db.shared[i]
        assert 0.20 <= (g == 1).mean() <= 0.30 and 0.04 <= (g == 2).mean() <= 0.06, i
        assert db.low_complexity[i].mean() >= 0.05
        assert db.parent_vi[vi] in db.genus_vi
    lc_total = sum(int(m.sum()) for m in db.low_complexity) / sum(len(g) for g in db.genomes)
    assert lc_total >= 0.05
    for j in range(len(db.strain_vi)):
        diff = (db.genomes[len(db.species_vi) - len(db.strain_vi) + j] != db.genomes[0]).mean()
        assert 0 < diff <= 0.01
    # a store built from the regions by the oracle's DBGoal restatement: shared k-mers go to the genus / the root
    seq, off, nvi = db.regions()
    b = orc.DbBuild(31, db.n_values, db.parent_vi)
    b.fill(seq, off, nvi)
    b.optimize()
    b.update(seq, off, nvi)
    kmers, vidx = b.fetch()
    counts = np.bincount(vidx, minlength=db.n_values)
    assert counts[0] > 1000 and all(counts[g] > 10_000 for g in db.genus_vi) and counts[db.dominant_vi] > 1500
    pad = np.arange(1 + len(db.genus_vi), db.species_vi[0])
    assert len(pad) == 90 - 1 - 3 - len(db.species_vi) - 1 and counts[pad].sum() == 0  # the padding nodes have no k-mers
    # the same seed gives the same genomes
    again = synth.SkewedDB(genera=3, species_per_genus=3, genome_len=60_000, strains=2, dominant_len=2000, n_values=90, seed=4)
    assert all(np.array_equal(a, b) for a, b in zip(db.genomes, again.genomes))


def _store(db, k=31):
    seq, off, nvi = db.regions()
    b = orc.DbBuild(k, db.n_values, db.parent_vi)
    b.fill(seq, off, nvi)
    b.optimize()
    b.update(seq, off, nvi)
    kmers, vidx = b.fetch()
    return orc.DB(k, kmers, vidx, db.n_values, db.parent_vi)


def test_skewed_read_mixes_hold_their_proportions(skew):
    db = skew
    n = 40_000
    odb = _store(db)
    seq, off, info = synth.skewed_reads(db, n, "dominated", seed=3)
    assert abs((info["src"] == len(db.genomes) - 1).mean() - 0.9) < 0.01
    run = orc.MatchRun(odb)
    cv, fl = run.submit(seq, off, threads=4)
    t, _ = run.finish()
    assert t[db.dominant_vi, orc.C_READS] >= 0.85 * t[:, orc.C_READS].sum()
    seq, off, info = synth.skewed_reads(db, n, "background", seed=3)
    assert abs((info["src"] < 0).mean() - 0.95) < 0.01
    cv, fl = orc.MatchRun(odb).submit(seq, off, threads=4)
    assert np.all(fl[info["src"] < 0] & orc.F_FOUND == 0)  # the random reads hit nothing
    assert abs((fl & orc.F_FOUND == 0).mean() - 0.95) < 0.01
    cuts = (13_001, 29_500)
    seq, off, info = synth.skewed_reads(db, n, "ragged", seed=3, cuts=cuts)
    L = np.diff(off.astype(np.int64))
    assert L.min() >= 35 and L.max() <= 450
    assert 0.08 <= (L > 151).mean() <= 0.12 and (L < 152).mean() >= 0.85
    assert 0.015 <= info["has_n"].mean() <= 0.03 and info["lower"].any()
    reads = [seq[off[i]:off[i + 1]].tobytes() for i in range(n)]
    nr = [r for r in reads if b"N" in r or b"n" in r]
    runs = [len(x) for r in nr for x in r.upper().replace(b"A", b" ").replace(b"C", b" ").replace(b"G", b" ").replace(b"T", b" ").split()]
    assert max(runs) <= 40 and min(runs) >= 1
    assert any(r != r.upper() for r in reads)
    d = np.flatnonzero(info["dup_of"] >= 0)
    assert 0.04 <= len(d) / n <= 0.06
    assert all(reads[i] == reads[info["dup_of"][i]] and info["dup_of"][i] < i for i in d)
    for c in cuts:  # duplicates across every cut
        assert any(info["dup_of"][i] < c <= i for i in d)
    seq2, off2, _ = synth.skewed_reads(db, n, "ragged", seed=3, cuts=cuts)
    assert np.array_equal(seq, seq2) and np.array_equal(off, off2)
    seq, off, info = synth.skewed_reads(db, 30_000, "combined", seed=2, cuts=(25_000,))
    assert len(off) == 30_001 and (info["src"] < 0).mean() > 0.25 and (info["dup_of"] >= 0).any()
    d = np.flatnonzero(info["dup_of"] >= 0)
    assert all(seq[off[i]:off[i + 1]].tobytes() == seq[off[j]:off[j + 1]].tobytes() for i, j in zip(d, info["dup_of"][d]))
