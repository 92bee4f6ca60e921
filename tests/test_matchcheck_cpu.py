"""The whole-result checker (tests/matchcheck.py) and the oracle's per-read dtable terms it rests on: the oracle's own
double table passes, on the reference's golden vectors and on a randomised batch, and a double table that leaves one
read's term out or adds it twice fails.  CPU only."""
import os

import numpy as np
import pytest

import matchcheck
from conftest import GOLDEN
from oracle import gs_oracle as orc


def _run(db, seq, off, threads=1, first_read_no=0, **cfg):
    run = orc.MatchRun(db, **cfg)
    cv, fl, terms = run.submit_terms(seq, off, first_read_no, threads)
    t, d = run.finish()
    return dict(table=t, dtable=d, class_vi=cv, flags=fl, terms=terms)


def _dengue():
    lines = open(os.path.join(GOLDEN, "dengue1", "dengue1.fasta")).read().split("\n")
    genome = "".join(l.strip() for l in lines if not l.startswith(">")).upper()
    keys = np.unique(orc.canonical_kmers(genome, 31))
    return genome, orc.DB(31, keys, np.zeros(len(keys), np.int32), 1, np.array([-1], np.int32))


def _random_store(rng, k=21, n_gen=6):
    """root 0, genera 1..2, species 3..: random genomes with a shared block per genus, k-mer -> LCA (DbBuild)"""
    parent = np.array([-1, 0, 0] + [1 + i % 2 for i in range(n_gen)], dtype=np.int32)
    core = [rng.choice(list(b"ACGT"), 800).astype(np.uint8) for _ in range(2)]
    genomes = []
    for i in range(n_gen):
        g = rng.choice(list(b"ACGT"), 4000).astype(np.uint8)
        g[1000:1800] = core[i % 2]
        genomes.append(g)
    seq = np.concatenate(genomes)
    off = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.uint64)
    b = orc.DbBuild(k, len(parent), parent)
    b.fill(seq, off, np.arange(3, 3 + n_gen, dtype=np.int32))
    b.optimize()
    b.update(seq, off, np.arange(3, 3 + n_gen, dtype=np.int32))
    kmers, vidx = b.fetch()
    b.close()
    return genomes, orc.DB(k, kmers, vidx, len(parent), parent)


def _random_reads(rng, genomes, n):
    reads = []
    for _ in range(n):
        g = genomes[int(rng.integers(0, len(genomes)))]
        L = int(rng.integers(15, 400))
        p = int(rng.integers(0, len(g) - L))
        r = bytearray(g[p:p + L].tobytes())
        for _ in range(int(rng.integers(0, 6))):
            r[int(rng.integers(0, L))] = int(rng.choice(list(b"ACGTN")))
        reads.append(bytes(r))
    return orc.pack_reads(reads)


def test_oracle_dtable_passes_on_the_golden_vectors():
    genome, db = _dengue()
    rd = orc.parse_fastq(open(os.path.join(GOLDEN, "dengue1", "test.fastq"), "rb").read(), k=31)
    o = _run(db, rd["seq"], rd["seq_off"])
    matchcheck.check_match(o, dict(o))
    reads = [genome[i:i + 150] for i in range(0, len(genome) - 150, 37)] + [genome]
    seq, off = orc.pack_reads(reads)
    o = _run(db, seq, off, max_read_tax_err=0.5)
    assert int(o["table"][0, orc.C_READS]) > 100
    assert matchcheck.check_match(o, dict(o)) <= 1.0


@pytest.mark.parametrize("threads", [1, 8])
def test_oracle_dtable_passes_on_a_random_batch(threads):
    rng = np.random.default_rng(7)
    genomes, db = _random_store(rng)
    seq, off = _random_reads(rng, genomes, 5000)
    o = _run(db, seq, off, threads=threads, first_read_no=123)
    counted = o["flags"] & orc.F_COUNTED != 0
    assert counted.sum() > 3000 and np.array_equal(counted, o["terms"][:, orc.T_CN] >= 0)
    assert np.array_equal(o["terms"][counted, orc.T_CN], o["class_vi"][counted])
    assert (o["terms"][:, orc.T_TAX_ERR] > 0).sum() > 500  # some terms are not zero
    matchcheck.check_match(o, dict(o))
    # the terms are the reference's: err = tax_err / max, the integers are those of the integer table's READS column
    assert np.array_equal(np.bincount(o["terms"][counted, orc.T_CN], minlength=db.n_values), o["table"][:, orc.C_READS])


def _nonzero_read(o):
    t = o["terms"]
    return int(np.flatnonzero((t[:, orc.T_CN] >= 0) & (t[:, orc.T_TAX_ERR] > 0) & (t[:, orc.T_CLASS_ERR] > 0))[0])


@pytest.mark.parametrize("how", ["left_out", "twice"])
def test_a_dtable_off_by_one_read_fails(how):
    rng = np.random.default_rng(8)
    genomes, db = _random_store(rng)
    seq, off = _random_reads(rng, genomes, 3000)
    o = _run(db, seq, off)
    r = _nonzero_read(o)
    v, tax, cls, mx = (int(x) for x in o["terms"][r])
    t, c = tax / mx, cls / mx
    for j, term in enumerate((t, t * t, c, c * c)):
        g = dict(o, dtable=o["dtable"].copy())
        g["dtable"][v, j] += -term if how == "left_out" else term
        with pytest.raises(AssertionError, match="outside the bound"):
            matchcheck.check_match(o, g)
    # the same read's term in the wrong row
    other = int(np.flatnonzero((o["table"][:, orc.C_READS] > 0) & (np.arange(db.n_values) != v))[0])
    g = dict(o, dtable=o["dtable"].copy())
    g["dtable"][v, 0] -= t
    g["dtable"][other, 0] += t
    with pytest.raises(AssertionError):
        matchcheck.check_match(o, g)


def test_an_empty_cell_must_be_exactly_zero_and_the_integers_exact():
    rng = np.random.default_rng(9)
    genomes, db = _random_store(rng)
    seq, off = _random_reads(rng, genomes, 2000)
    o = _run(db, seq, off)
    empty = np.flatnonzero(o["table"][:, orc.C_READS] == 0)
    assert empty.size
    g = dict(o, dtable=o["dtable"].copy())
    g["dtable"][empty[0], 3] = 5e-324
    with pytest.raises(AssertionError, match="should be 0.0"):
        matchcheck.check_match(o, g)
    for col in (orc.C_MAX_CONTIG_READ_NO, orc.C_UNIQUE_KMERS):
        g = dict(o, table=o["table"].copy())
        g["table"][int(np.argmax(o["table"][:, orc.C_READS])), col] += 1
        with pytest.raises(AssertionError, match="table differs"):
            matchcheck.check_match(o, g)
    g = dict(o, flags=o["flags"].copy())
    g["flags"][5] ^= orc.F_COUNTED
    with pytest.raises(AssertionError, match="flags differs"):
        matchcheck.check_match(o, g)


def _parts(db, seq, off, cut):
    """the batch as two runs over its halves (read numbers kept): per-part results and the whole run's oracle"""
    o = _run(db, seq, off)
    parts = []
    for a, b in ((0, cut), (cut, len(off) - 1)):
        s0 = int(off[a])
        p = _run(db, seq[s0:int(off[b])], off[a:b + 1] - np.uint64(s0), first_read_no=a, count_unique=True)
        parts.append(p)
    return o, parts


def test_summed_parts_pass_and_a_term_dropped_or_doubled_across_parts_fails():
    rng = np.random.default_rng(10)
    genomes, db = _random_store(rng)
    seq, off = _random_reads(rng, genomes, 4000)
    o, parts = _parts(db, seq, off, 1700)
    # (two oracle runs each count the unique k-mers they see, which overlap: the integer table is held to the merged one)
    whole = dict(o, table=matchcheck.merge_tables([p["table"] for p in parts]))
    assert np.array_equal(whole["table"][:, orc.C_READS], o["table"][:, orc.C_READS])
    assert matchcheck.check_match_parts(whole, parts) <= 1.0
    r = _nonzero_read(parts[0])
    v, tax, cls, mx = (int(x) for x in parts[0]["terms"][r])
    t, c = tax / mx, cls / mx
    for j, term in enumerate((t, t * t, c, c * c)):
        dropped = [dict(parts[0], dtable=parts[0]["dtable"].copy()), parts[1]]
        dropped[0]["dtable"][v, j] -= term
        with pytest.raises(AssertionError, match="outside the bound"):
            matchcheck.check_match_parts(whole, dropped)
        doubled = [parts[0], dict(parts[1], dtable=parts[1]["dtable"].copy())]
        doubled[1]["dtable"][v, j] += term  # the same read counted in the other part as well
        with pytest.raises(AssertionError, match="outside|should be 0.0"):
            matchcheck.check_match_parts(whole, doubled)
    # per-read outputs are concatenated in part order
    swapped = [parts[1], parts[0]]
    with pytest.raises(AssertionError):
        matchcheck.check_match_parts(whole, swapped)


def test_oracle_files_equals_one_run_over_the_records(tmp_path):
    """plain, gzip and BGZF FASTQ, multi-line FASTQ and FASTA: the same records in file order, read numbers running on"""
    import gzip

    from conftest import bgzf
    rng = np.random.default_rng(11)
    genomes, db = _random_store(rng)
    seq, off = _random_reads(rng, genomes, 900)
    reads = [seq[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(off) - 1)]
    fq = lambda rs, base: b"".join(b"@r%d\n%s\n+\n%s\n" % (base + i, r, b"F" * len(r)) for i, r in enumerate(rs))
    ml = lambda rs: b"".join(b"@m\n%s\n%s\n+\n%s\n%s\n" % (r[:20], r[20:], b"F" * 20, b"F" * (len(r) - 20)) for r in rs)
    fa = lambda rs: b"".join(b">f\n%s\n%s\n" % (r[:33], r[33:]) for r in rs)
    chunks = [reads[i * 150:(i + 1) * 150] for i in range(6)]
    files = [("a.fq", fq(chunks[0], 0)), ("b.fq.gz", gzip.compress(fq(chunks[1], 150))), ("c.fq.gz", bgzf(fq(chunks[2], 300))),
             ("d.fq", ml([r for r in chunks[3] if len(r) > 20])), ("e.fa", fa([r for r in chunks[4] if len(r) > 33])),
             ("f.fa.gz", bgzf(fa([r for r in chunks[5] if len(r) > 33])))]
    paths = []
    for name, data in files:
        paths.append(str(tmp_path / name))
        open(paths[-1], "wb").write(data)
    got = matchcheck.oracle_files(db, paths, threads=4, first_read_no=7, max_counts=True, max_kmer_res_counts=2)
    kept = chunks[0] + chunks[1] + chunks[2] + [r for r in chunks[3] if len(r) > 20] + [r for c in chunks[4:] for r in c if len(r) > 33]
    s, o = orc.pack_reads(kept)
    run = orc.MatchRun(db, max_kmer_res_counts=2)
    cv, fl, terms = run.submit_terms(s, o, 7, threads=4)
    t, d = run.finish()
    assert got["reads"] == len(kept) and got["bps"] == sum(len(r) for r in kept)
    assert np.array_equal(got["table"], t) and np.array_equal(got["class_vi"], cv) and np.array_equal(got["flags"], fl)
    assert np.array_equal(got["terms"], terms) and np.array_equal(got["max_counts"], run.max_counts())
    matchcheck.check_match(got, dict(table=t, dtable=d, class_vi=cv, flags=fl))
