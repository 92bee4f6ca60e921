"""The error gates and error sums of a batch of one read length, at every gate setting and at the edges of the FIXED loop.

A batch of one read length with 65 .. 128 k-mer positions (gs_match_submit_fixed, the FIXED loop of gs_match_kernel) takes both
error gates (max_read_tax_err, max_read_class_err) and both error quotients from a table that gs_api.cpp builds per (positions, gate
settings) and uploads once (GsQuotTable); every other batch computes them per read, and reads whose statistics are deferred into
records (stores of more than GS_NV_LDS values) get their quotients in gs_stat_reduce_kernel.  All of them must give what the oracle
gives: integer table, class_vi and flags bit for bit, every cell of the double table within tests/matchcheck.py's bound of the exact
sum of the oracle's terms.  Every case is submitted with submit_fixed and again with an offsets array (the general loop); the two
must give the same integer table.

Reads (n = 4000 per case, in turns): from the store's genomes with 0, 1, 5 and 30 substitutions, the same with an N at base 0, at
base max - 2, at base max - 1 and in the last base (max = L - k + 1; the first two count as bad bases below the last window, the
others as one behind them), and background.  That spreads tax_err and class_err from 0 to max.  Needs an MI355X: run with -m gpu."""
import itertools

import numpy as np
import pytest

import genestrip_amd as ga
from genestrip_amd import synth
import matchcheck
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

N_READS = 4000
GATES = (-1.0, 0.0, 0.1, 0.5, 1.0, 3.0)  # off, nothing allowed, fractions of max, 1 (the boundary between the two forms), absolute
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _reads(db, L, n, seed):
    """n reads of L bases back to back, read i of kind i % 9 (see the module docstring)"""
    k = db.k
    mx = L - k + 1
    rng = np.random.default_rng(seed)
    seq, off = synth.reads_host(db.genomes, n, read_len=L, seed=seed)
    seq = seq.copy().reshape(n, L)
    kind = np.arange(n) % 9
    subs = (0, 1, 5, 30)
    for i in range(n):  # substitutions: read i gets subs[(i // 9) % 4] of them at distinct places, each to another base
        s = subs[(i // 9) % 4]
        if s and kind[i] != 8:
            pos = rng.choice(L, size=s, replace=False)
            code = np.searchsorted(ACGT, seq[i, pos])
            seq[i, pos] = ACGT[(code + rng.integers(1, 4, s)) % 4]
    bg = kind == 8
    seq[bg] = ACGT[rng.integers(0, 4, (int(bg.sum()), L))]
    if mx >= 3:
        seq[kind == 4, 0] = ord("N")
        seq[kind == 5, mx - 2] = ord("N")
        seq[kind == 6, mx - 1] = ord("N")
        seq[kind == 7, L - 1] = ord("N")
    return seq.reshape(-1), off


class _Store:
    def __init__(self, db):
        self.db = db
        self.odb = orc.DB(db.k, db.kmers, db.value_idx, db.n_values, db.parent_vi)
        self.store = ga.DeviceKMerStore(db.k, db.kmers, db.value_idx, db.n_values, db.parent_vi)
        self._reads = {}

    def reads(self, L):
        if L not in self._reads:
            self._reads[L] = _reads(self.db, L, N_READS, seed=77 * self.db.k + L)
        return self._reads[L]

    def close(self):
        self.store.close()


@pytest.fixture(scope="module")
def s31():
    s = _Store(synth.SynthDB(k=31, genera=3, species_per_genus=5, genome_len=20000, seed=21))
    assert s.db.n_values == 19
    yield s
    s.close()


@pytest.fixture(scope="module")
def s25():
    s = _Store(synth.SynthDB(k=25, genera=3, species_per_genus=5, genome_len=20000, seed=22))
    yield s
    s.close()


@pytest.fixture(scope="module")
def s31_records():
    """more than 128 values: counters in global memory, reads of one tax id deferred into records"""
    s = _Store(synth.SynthDB(k=31, genera=13, species_per_genus=10, genome_len=4000, seed=23))
    assert s.db.n_values > 128
    yield s
    s.close()


def _check(s, L, **cfg):
    """one length at one setting: fixed and offsets-array submit against the oracle and each other; returns the oracle's result"""
    n = N_READS
    seq, off = s.reads(L)
    what = f"k {s.db.k} L {L} {cfg}"
    o = matchcheck.oracle_batch(s.odb, seq, off, **cfg)
    ref = matchcheck.dtable_reference(o["terms"], s.db.n_values)
    m = ga.FastqKMerMatcher(s.store, ga.MatchConfig(**cfg))
    try:
        cv_a, fl_a = m.match_reads(seq, off)
        t_a, d_a = m.finish()
        m.reset()
        cv_f, fl_f = np.full(n, -7, dtype=np.int32), np.full(n, 0xee, dtype=np.uint8)
        m.submit_fixed(seq, L, n, class_vi=cv_f, flags=fl_f)
        t_f, d_f = m.finish()
    finally:
        m.close()
    r_a = matchcheck.check_match(o, dict(table=t_a, dtable=d_a, class_vi=cv_a, flags=fl_a), what + " offsets array", ref=ref)
    r_f = matchcheck.check_match(o, dict(table=t_f, dtable=d_f, class_vi=cv_f, flags=fl_f), what + " fixed", ref=ref)
    print(f"{what}: counted {int(o['table'][:, orc.C_READS].sum())} of {n}, worst dtable ratio offsets {r_a:.3f} fixed {r_f:.3f}")
    assert np.array_equal(t_f, t_a), what + ": integer tables of the two submits differ"
    return o


def _spread(o, mx):
    """the counted reads of an ungated run cover tax_err and class_err from 0 up to nearly max"""
    t = o["terms"][o["terms"][:, orc.T_CN] >= 0]
    te, ce = t[:, orc.T_TAX_ERR], t[:, orc.T_CLASS_ERR]
    assert te.min() == 0 and ce.min() == 0
    assert te.max() >= mx - 2 and ce.max() >= mx - 2, (int(te.max()), int(ce.max()), mx)
    assert len(np.unique(te)) >= 20 and len(np.unique(ce)) >= 20


EDGE_GATES = ((-1.0, -1.0), (0.1, 0.5), (3.0, 1.0))


@pytest.mark.parametrize("L", [128, 150, 158, 127, 159])
def test_lengths_at_the_edges_k31(s31, L):
    """k = 31 (k folded in at compile time): 98, 120 and 128 positions take the FIXED loop, 127 bases the general loop, 159 bases
    (129 positions) the wide kernel"""
    for tax, cls in EDGE_GATES:
        o = _check(s31, L, max_read_tax_err=tax, max_read_class_err=cls)
        if tax < 0 and cls < 0:
            _spread(o, L - 31 + 1)


@pytest.mark.parametrize("L", [128, 152])
def test_lengths_at_the_edges_k25(s25, L):
    """k = 25 (the any-k instantiation, KC = 0): 104 and 128 positions, both in the FIXED loop"""
    for tax, cls in EDGE_GATES:
        o = _check(s25, L, max_read_tax_err=tax, max_read_class_err=cls)
        if tax < 0 and cls < 0:
            _spread(o, L - 25 + 1)


@pytest.mark.parametrize("tax", GATES)
def test_every_gate_setting(s31, tax):
    """every pair of the two gates' settings at 150 bases; a wider class gate never counts fewer reads, and with the tax gate off it
    does take reads away (the oracle's counts: the cases do reach the gates)"""
    counted = []
    for cls in GATES:
        o = _check(s31, 150, max_read_tax_err=tax, max_read_class_err=cls)
        counted.append(int(o["table"][:, orc.C_READS].sum()))
    off_, zero, tenth, half, one, three = counted
    assert off_ >= half >= tenth >= zero > 0  # (fractions of max: 0 <= 0.1 <= 0.5)
    assert off_ >= three >= one >= zero       # (1 and 3: absolute counts, or the whole of max)
    if tax < 0:
        assert off_ > half > tenth > zero


def test_every_gate_setting_record_tier(s31_records):
    """stores of more than 128 values: the gates of the FIXED loop feed the deferred records, whose quotients gs_stat_reduce_kernel
    forms; every value of each gate occurs once"""
    for i, tax in enumerate(GATES):
        _check(s31_records, 150, max_read_tax_err=tax, max_read_class_err=GATES[(i + 2) % len(GATES)])


@pytest.mark.parametrize("L", [128, 158, 127, 159])
def test_lengths_at_the_edges_record_tier(s31_records, L):
    o = _check(s31_records, L)
    _spread(o, L - 31 + 1)
    _check(s31_records, L, max_read_tax_err=0.5, max_read_class_err=0.1)


def test_threshold_above_one(s31):
    """threshold > 1: read_kmers is summed over the distinct nodes of the read before it indexes the table"""
    _check(s31, 150, threshold=4, max_paths=3, max_read_tax_err=0.5, max_read_class_err=0.5)
    _check(s31, 158, threshold=4, max_paths=3)


@pytest.mark.parametrize("tier", ["lds", "records"])
def test_three_submits_of_one_run_150_140_150(s31, s31_records, tier):
    """one run, batches of 150, 140 and 150 bases: the table is built, rebuilt for the other length and rebuilt again; the sums over
    all three batches are the oracle's"""
    s = s31 if tier == "lds" else s31_records
    cfg = dict(max_read_tax_err=0.1, max_read_class_err=0.5)
    n = N_READS
    orun = orc.MatchRun(s.odb, **cfg)
    m = ga.FastqKMerMatcher(s.store, ga.MatchConfig(**cfg))
    ocv, ofl, terms, gcv, gfl = [], [], [], [], []
    try:
        for b, L in enumerate((150, 140, 150)):
            seq, off = _reads(s.db, L, n, seed=900 + b)
            cv, fl, te = orun.submit_terms(seq, off, b * n, threads=8)
            ocv.append(cv)
            ofl.append(fl)
            terms.append(te)
            cv_f, fl_f = np.full(n, -7, dtype=np.int32), np.full(n, 0xee, dtype=np.uint8)
            m.submit_fixed(seq, L, n, first_read_no=b * n, class_vi=cv_f, flags=fl_f)
            gcv.append(cv_f)
            gfl.append(fl_f)
        ot, od = orun.finish()
        gt, gd = m.finish()
    finally:
        m.close()
        orun.close()
    o = dict(table=ot, dtable=od, terms=np.concatenate(terms), class_vi=np.concatenate(ocv), flags=np.concatenate(ofl))
    assert 0 < int(ot[:, orc.C_READS].sum()) < 3 * n
    matchcheck.check_match(o, dict(table=gt, dtable=gd, class_vi=np.concatenate(gcv), flags=np.concatenate(gfl)), f"150, 140, 150 ({tier})")
