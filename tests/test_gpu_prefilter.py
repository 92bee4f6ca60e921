"""The sampled 15-mer prefilter in front of the FIXED loop of gs_match_kernel (genestrip_amd/csrc/gs_prefilter.hip): every case runs
with the prefilter forced on (GS_PREFILTER=1), forced off (GS_PREFILTER=0) and through the CPU oracle.  Integer table (max keys and
unique counts are columns of it), class_vi and flags of every read are identical in all three; the double tables are within
matchcheck's bound of the exact sums and of each other (check_dtables_agree: what two summation orders may differ by).
Every forced-on run asserts through prefilter_info() that the filter exists and that the batch went through it; where there is
background, at least 90 % of it was rejected (uniform background against these small stores: ~97 % by tests/prefilter.py).
Needs an MI355X: run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import genestrip_amd as ga
from genestrip_amd import synth
import matchcheck
import prefilter as pf
from oracle import gs_oracle as orc
from prefilter import make_reads

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _reads(genomes, L, n, seed, background="odd"):
    """n reads of L bases: genome windows with ~1 % substitutions; background "odd": every second read uniform random, "all", "none" """
    rng = np.random.default_rng(seed)
    g = rng.integers(0, genomes.shape[0], n)
    p = rng.integers(0, genomes.shape[1] - L + 1, n)
    seq = np.ascontiguousarray(genomes[g[:, None], p[:, None] + np.arange(L)[None, :]], dtype=np.uint8)
    sub = rng.random((n, L)) < 0.01
    seq[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    bg = np.zeros(n, dtype=bool)
    if background == "odd":
        bg[1::2] = True
    elif background == "all":
        bg[:] = True
    seq[bg] = ACGT[rng.integers(0, 4, (int(bg.sum()), L))]
    return seq, bg


class _Store:
    def __init__(self, k, kmers, vidx, n_values, parent_vi):
        self.k = k
        self.odb = orc.DB(k, kmers, vidx, n_values, parent_vi)
        self.dev = ga.DeviceKMerStore(k, kmers, vidx, n_values, parent_vi)

    def close(self):
        self.dev.close()


def _device(store, mode, batches, L, want_out=True, **cfg):
    """one run over `batches` = [(seq, n, first)], begun under GS_PREFILTER = mode (None: the rules decide; the library reads the
    variable when a run begins); returns the result and the prefilter_info() behind every batch"""
    before = os.environ.pop("GS_PREFILTER", None)
    if mode is not None:
        os.environ["GS_PREFILTER"] = str(mode)
    try:
        m = ga.FastqKMerMatcher(store.dev, ga.MatchConfig(**cfg))
    finally:
        os.environ.pop("GS_PREFILTER", None)
        if before is not None:
            os.environ["GS_PREFILTER"] = before
    try:
        cvs, fls, infos = [], [], []
        for seq, n, first in batches:
            cv = np.full(n, -7, dtype=np.int32) if want_out else None
            fl = np.full(n, 0xee, dtype=np.uint8) if want_out else None
            m.submit_fixed(np.ascontiguousarray(seq).reshape(-1), L, n, first, class_vi=cv, flags=fl)
            infos.append(m.prefilter_info())
            cvs.append(cv)
            fls.append(fl)
        t, d = m.finish()
    finally:
        m.close()
    return dict(table=t, dtable=d, class_vi=np.concatenate(cvs) if want_out else None, flags=np.concatenate(fls) if want_out else None), infos


def _check(store, seq, L, n, what, first=0, bg=None, want_out=True, **cfg):
    seq = np.ascontiguousarray(seq).reshape(-1, L)[:n]
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    o = matchcheck.oracle_batch(store.odb, seq.reshape(-1), off, first_read_no=first, **cfg)
    on, info_on = _device(store, 1, [(seq, n, first)], L, want_out, **cfg)
    offr, info_off = _device(store, 0, [(seq, n, first)], L, want_out, **cfg)
    matchcheck.check_match(o, on, what + " prefilter on")
    matchcheck.check_match(o, offr, what + " prefilter off")
    assert np.array_equal(on["table"], offr["table"]), what
    matchcheck.check_dtables_agree(on["dtable"], offr["dtable"], on["table"][:, orc.C_READS], what + ": double tables on / off")
    i = info_on[0]
    assert i["built"] and i["n_lmers"] > 0 and i["reads"] == n and 0 <= i["survivors"] <= n, i
    assert info_off[0]["survivors"] == -1
    found = (np.asarray(o["flags"]) & orc.F_FOUND) != 0
    assert i["survivors"] >= int(found.sum())
    if bg is not None and bg[:n].any():
        n_bg = int(bg[:n].sum())
        assert not found[bg[:n]].any()
        assert i["survivors"] - int(found.sum()) <= n_bg // 10, (i, n_bg)  # at least 90 % of the background was rejected
    return o, i


@pytest.fixture(scope="module")
def db31():
    return synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)


@pytest.fixture(scope="module")
def st31(db31):
    s = _Store(31, db31.kmers, db31.value_idx, db31.n_values, db31.parent_vi)
    yield s
    s.close()


@pytest.fixture(scope="module")
def mix31(db31):
    return _reads(db31.genomes, 150, 4097, seed=150)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_sizes(st31, mix31, n):
    seq, bg = mix31
    _check(st31, seq, 150, n, f"{n} reads", bg=bg)


def test_filter_is_the_restatements_set(st31, db31, mix31):
    """|S| by the popcount of the exact level, and the survivors read for read, against tests/prefilter.py"""
    seq, bg = mix31
    S = pf.lmer_set(db31.kmers, 31)
    _, info = _device(st31, 1, [(seq, 4097, 0)], 150)
    assert info[0]["n_lmers"] == len(S)
    assert info[0]["survivors"] == int(pf.passes(S, seq, 150, 31).sum())


@pytest.mark.parametrize("kind", ["all", "none", "odd"], ids=["all_background", "all_genome", "half_and_half"])
def test_streams(st31, db31, kind):
    seq, bg = _reads(db31.genomes, 150, 3001, seed=7, background=kind)
    o, i = _check(st31, seq, 150, 3001, kind, bg=bg)
    if kind == "all":  # (no survivor at all is not promised: a count of 0 is what test_no_survivor pins)
        assert i["survivors"] <= 300 and not np.any(o["table"][:, orc.C_READS])
    if kind == "none":
        assert i["survivors"] > 2900


def test_no_survivor(st31):
    """a batch of one base repeated: no sample is in S, the match kernel runs on a list of 0 reads"""
    seq = np.full((500, 150), ord("N"), dtype=np.uint8)
    o, i = _check(st31, seq, 150, 500, "no survivor")
    assert i["survivors"] == 0 and np.all(o["class_vi"] == -1) and not np.any(o["flags"])


@pytest.mark.parametrize("want_out", [False, True], ids=["no_outputs", "outputs"])
@pytest.mark.parametrize("unique", [False, True], ids=["no_unique", "unique"])
def test_first_read_no_unique_and_outputs(st31, mix31, unique, want_out):
    seq, bg = mix31
    o, _ = _check(st31, seq, 150, 2000, f"unique {unique} outputs {want_out}", first=2 ** 33 + 5, bg=bg, want_out=want_out,
                  count_unique=unique)
    t = o["table"]
    assert np.all(t[t[:, orc.C_MAX_CONTIG_LEN] > 0, orc.C_MAX_CONTIG_READ_NO] >= 2 ** 33 + 5)
    assert np.all(t[:, orc.C_UNIQUE_KMERS] >= 0) if unique else np.all(t[:, orc.C_UNIQUE_KMERS] == -1)


_GLOBAL_STATS = """
import test_gpu_prefilter as t
from genestrip_amd import synth
db = synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)
s = t._Store(31, db.kmers, db.value_idx, db.n_values, db.parent_vi)
seq, bg = t._reads(db.genomes, 150, 4097, seed=150)
t._check(s, seq, 150, 4097, "global statistics", bg=bg)
s.close()
print("global statistics ok")
"""


def test_global_statistics_instantiation():
    """GS_FORCE_GLOBAL_STATS=1: gs_match_kernel<false, ..> (counters in global memory, deferred records) takes the list too.  The
    launchers read the variable once per process, so the case runs in a process of its own"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, GS_FORCE_GLOBAL_STATS="1", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    r = subprocess.run([sys.executable, "-s", "-c", _GLOBAL_STATS], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "global statistics ok" in r.stdout, (r.stdout[-800:], r.stderr[-3000:])


@pytest.mark.parametrize("k,L", [(31, 128), (31, 158), (25, 128), (25, 150), (25, 152)])
def test_lengths_and_k(k, L):
    """the reads of the CPU list: both strands, substitutions, N, lower case, CR, and the two reads whose only clean k-mer is the
    first / the last one"""
    db = synth.SynthDB(k=k, genera=2, species_per_genus=3, genome_len=20000, seed=3)
    s = _Store(k, db.kmers, db.value_idx, db.n_values, db.parent_vi)
    try:
        n = 1500
        seq = make_reads(db.genomes, L, k, n, seed=100 * k + L)
        o, _ = _check(s, seq, L, n, f"k {k} L {L}", bg=np.arange(n) % 4 == 3)
        assert o["flags"][0] & orc.F_FOUND and o["flags"][1] & orc.F_FOUND
    finally:
        s.close()


def test_skewed_store_with_overflow_table():
    """a store whose k-mers partly live in the overflow table (strains: more windows per minimizer than record buckets)"""
    sdb = synth.SkewedDB(genera=3, species_per_genus=4, genome_len=150_000, strains=2, dominant_len=1000, n_values=70, seed=11)
    seq, off, nvi = sdb.regions()
    b = orc.DbBuild(31, sdb.n_values, sdb.parent_vi)
    b.fill(seq, off, nvi)
    b.optimize()
    b.update(seq, off, nvi)
    kmers, vidx = b.fetch()
    b.close()
    s = _Store(31, kmers, vidx, sdb.n_values, sdb.parent_vi)
    try:
        info = s.dev.info
        assert info.n_in_records < info.n_stored  # the overflow table is in use
        parts = [synth.skewed_reads(sdb, 1500, mix, seed=5)[0] for mix in ("dominated", "background")]
        reads = np.concatenate(parts).reshape(-1, 150)
        _check(s, reads, 150, len(reads), "skewed store")
    finally:
        s.close()


def test_feedback_rule_switches_between_two_batches(st31, db31):
    """under the rules (GS_PREFILTER unset) a batch of genome reads goes through the prefilter, nearly all of it survives, and the
    next batch of the run goes straight to the match kernel; the result is that of both batches either way"""
    a, _ = _reads(db31.genomes, 150, 2000, seed=21, background="none")
    b, _ = _reads(db31.genomes, 150, 2000, seed=22, background="odd")
    both = np.concatenate([a, b])
    off = np.arange(4001, dtype=np.uint64) * np.uint64(150)
    o = matchcheck.oracle_batch(st31.odb, both.reshape(-1), off)
    res, infos = _device(st31, None, [(a, 2000, 0), (b, 2000, 2000)], 150)
    assert infos[0]["built"] and infos[0]["survivors"] > 1700 and infos[1]["survivors"] == -1, infos
    matchcheck.check_match(o, res, "feedback rule")
    forced, infos = _device(st31, 1, [(a, 2000, 0), (b, 2000, 2000)], 150)
    assert infos[1]["survivors"] >= 0
    matchcheck.check_match(o, forced, "two batches, forced on")
    assert np.array_equal(res["table"], forced["table"])
