"""Reads of one tax id leave the FIXED loop of gs_match_kernel (counters in LDS) as records that gs_sn_reduce_kernel works off, one
lane per record (GsSnRec, genestrip_amd/csrc/gs_snrec.h).  A read is deferred iff it has no byte that is no upper-case CGAT letter
and its hit k-mers all carry one tax id; every other read is booked by the wave that probed it.

Stores and reads are those of tests/test_gpu_single_node_reduce.py (k = 31, 19 values, read i of kind i % 14: genome reads with 0 .. 30
substitutions, of these with an N at base 0, max - 2, max - 1 and L - 1, background, and the directed reads whose runs end at 63,
start at 64, cross, end at max - 1 and cover the whole read), plus one store of 127 values, where the reduce kernel has four counter
copies, and one of 141 values, whose counters live in HBM (gs_match_kernel<false, ..>: nothing may be deferred).

Every case runs with GS_SN_DEFER=1 and =0 and, where said, with GS_PREFILTER=0 (slot = read number) and =1 (slot = index into the
survivor list), and holds the integer table, class_vi and flags of each run to the oracle bit for bit and the double table within
tests/matchcheck.py's bound.  sn_info() must report exactly the deferrable reads of the batch (counted here from the oracle's
segments) when deferral is on, and none when it is off or the counters live in HBM.
Needs an MI355X: run with -m gpu."""
import os

import numpy as np
import pytest

import genestrip_amd as ga
from genestrip_amd import synth
import matchcheck
from oracle import gs_oracle as orc
import test_gpu_single_node_reduce as base

pytestmark = pytest.mark.gpu

K = base.K
N = base.N_READS
CGAT = np.zeros(256, dtype=bool)
CGAT[list(b"ACGT")] = True


class _Env:
    """environment variables the library reads when a run begins"""

    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def base_db():
    db = synth.SynthDB(k=K, genera=3, species_per_genus=5, genome_len=20000)
    assert db.n_values == 19
    return db


@pytest.fixture(scope="module")
def stores(base_db):
    half = np.random.default_rng(5).random(len(base_db.kmers)) < 0.5
    s = dict(S1=base._Store(base_db), S2=base._Store(base_db, half),
             S3=base._Store(base_db, np.isin(base_db.value_idx, base_db.species_vi)))
    big = synth.SynthDB(k=K, genera=6, species_per_genus=20, genome_len=3000, seed=9)
    assert big.n_values == 127
    s["V127"] = base._Store(big)
    hbm = synth.SynthDB(k=K, genera=10, species_per_genus=13, genome_len=3000, seed=10)
    assert hbm.n_values == 141
    s["V141"] = base._Store(hbm)
    for x in s.values():
        x.cache = {}
    yield s
    for x in s.values():
        x.close()


def _deferrable(s, rows):
    """reads without a non-CGAT byte whose hit positions hold one node, from the oracle's segments"""
    n = 0
    for row in rows:
        if CGAT[row].all():
            n += len({code for code, _ in s.odb.segments(row.tobytes()) if code >= 0}) == 1
    return n


def _oracle(s, L, sel, batches, first, cfg):
    """the oracle's run over the batches (slices of the selected reads), once per (length, selection, batches, settings)"""
    key = (L, sel, tuple(batches), first, tuple(sorted(cfg.items())))
    if key not in s.cache:
        rows = _rows(s, L, sel)
        run = orc.MatchRun(s.odb, **cfg)
        cvs, fls, terms, no = [], [], [], first
        try:
            for a, b in batches:
                part = rows[a:b]
                cv, fl, te = run.submit_terms(part.reshape(-1), np.arange(len(part) + 1, dtype=np.uint64) * np.uint64(L), no, threads=8)
                cvs.append(cv), fls.append(fl), terms.append(te)
                no += len(part)
            t, d = run.finish()
        finally:
            run.close()
        o = dict(table=t, dtable=d, terms=np.concatenate(terms), class_vi=np.concatenate(cvs), flags=np.concatenate(fls))
        s.cache[key] = (o, matchcheck.dtable_reference(o["terms"], s.db.n_values), [_deferrable(s, rows[a:b]) for a, b in batches])
    return s.cache[key]


SELECTIONS = {
    "all": lambda kind: np.ones(len(kind), dtype=bool),
    "n": lambda kind: (kind >= 4) & (kind <= 7),    # an N at base 0, max - 2, max - 1, L - 1
    "directed": lambda kind: kind >= 9,            # runs that end at 63, start at 64, cross, end at max - 1, cover the read
}


def _rows(s, L, sel):
    seq, _ = s.reads(L)
    return np.ascontiguousarray(seq.reshape(N, L)[SELECTIONS[sel](np.arange(N) % base.N_KINDS)])


def _device(s, L, sel, batches, first, defer, pf, outputs, cfg):
    rows = _rows(s, L, sel)
    with _Env(GS_SN_DEFER=defer, GS_PREFILTER=pf):
        m = ga.FastqKMerMatcher(s.store, ga.MatchConfig(**cfg))
    cvs, fls, infos, no = [], [], [], first
    try:
        for a, b in batches:
            part = np.ascontiguousarray(rows[a:b])
            cv = np.full(len(part), -7, dtype=np.int32) if outputs else None
            fl = np.full(len(part), 0xee, dtype=np.uint8) if outputs else None
            m.submit_fixed(part.reshape(-1), L, len(part), first_read_no=no, class_vi=cv, flags=fl)
            infos.append((m.sn_info(), m.prefilter_info()))
            cvs.append(cv), fls.append(fl)
            no += len(part)
        t, d = m.finish()
    finally:
        m.close()
    g = dict(table=t, dtable=d, class_vi=np.concatenate(cvs) if outputs else None, flags=np.concatenate(fls) if outputs else None)
    return g, infos


def _check(s, L, sel="all", batches=None, first=0, pfs=(0, 1), outputs=True, lds=True, **cfg):
    """one case under GS_SN_DEFER = 1 and 0 and every GS_PREFILTER of pfs; returns the oracle's result and the deferrable counts"""
    n_sel = len(_rows(s, L, sel))
    batches = [(0, n_sel)] if batches is None else batches
    o, ref, want = _oracle(s, L, sel, batches, first, cfg)
    for pf in pfs:
        for defer in (1, 0):
            what = f"L {L} reads {sel} batches {batches} prefilter {pf} defer {defer} outputs {outputs} {cfg}"
            g, infos = _device(s, L, sel, batches, first, defer, pf, outputs, cfg)
            ratio = matchcheck.check_match(o, g, what, ref=ref)
            booked = [i["booked"] for i, _ in infos]
            print(f"{what}: booked {booked} of deferrable {want}, worst dtable ratio {ratio:.3f}")
            for (sn, pi), w in zip(infos, want):
                assert (pi["survivors"] >= 0) == bool(pf), (what, pi)  # the slot is the list index / the read number as intended
                if defer and lds:
                    assert sn["deferred"] and sn["booked"] == w, (what, sn, w)
                else:
                    assert not sn["deferred"] and sn["booked"] == 0, (what, sn)
    return o, want


@pytest.mark.parametrize("L", [128, 150, 158])
@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_lengths(stores, name, L):
    """98, 120 and 128 positions (at 128 word 1 is full), ungated and with both gates rejecting some reads"""
    o, want = _check(stores[name], L)
    found = int(np.count_nonzero(o["flags"] & orc.F_FOUND))
    assert 0 < want[0] <= found
    if name == "S3":  # species k-mers only: what hits and has no N is deferred, but for a handful of reads
        clean = CGAT[_rows(stores[name], L, "all")].all(axis=1)
        assert want[0] >= int(np.count_nonzero(clean & ((o["flags"] & orc.F_FOUND) != 0))) - N // 400
    o, _ = _check(stores[name], L, max_read_tax_err=0.1, max_read_class_err=0.5)
    counted = int(o["table"][:, orc.C_READS].sum())
    assert counted < found and (counted > 0 or name == "S2")  # (S2 holds half of the k-mers: every read misses more than a tenth)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches(stores, n):
    """fewer records than a wave has lanes, exactly as many, one more.  Reads 13 .. (kind 13: the whole read is one run)"""
    for name in ("S1", "S3"):
        _, want = _check(stores[name], 150, batches=[(13, 13 + n)])
        assert want[0] >= 1


def test_two_batches_second_smaller(stores):
    """one run, 2500 reads and then 1500: behind the second batch's records lie the first one's"""
    for name in ("S1", "S3"):
        _, want = _check(stores[name], 150, batches=[(0, 2500), (2500, N)], first=2 ** 33 + 5)
        assert want[0] > want[1] > 0


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_settings(stores, name):
    """outputs not asked for; thresholds 1 (test_lengths), 2, and above any read's count; no classification; gates that let nothing
    but error-free reads through"""
    s = stores[name]
    _check(s, 150, outputs=False)
    _check(s, 150, pfs=(1,), threshold=2)
    o, want = _check(s, 150, pfs=(1,), threshold=200)
    assert want[0] > 0 and int(o["table"][:, orc.C_READS].sum()) == 0 and not np.any(o["flags"] & orc.F_RETURNED)
    o, _ = _check(s, 150, pfs=(0,), classify=False)
    assert int(o["table"][:, orc.C_READS].sum()) == 0 and int(o["table"][:, orc.C_KMERS].sum()) > 0
    o, _ = _check(s, 150, pfs=(0,), max_read_tax_err=0.0, max_read_class_err=0.0)
    assert 0 < int(o["table"][:, orc.C_READS].sum()) or name == "S2"  # (S2 holds half of the k-mers: no read is error-free)
    _check(s, 150, pfs=(1,), outputs=False, max_read_tax_err=0.1, max_read_class_err=0.5)


@pytest.mark.parametrize("L", [128, 150, 158])
def test_reads_with_an_n_are_not_deferred(stores, L):
    """an N at base 0, max - 2, max - 1 or L - 1: most of these reads hit one species of S3, none leaves as a record"""
    o, want = _check(stores["S3"], L, sel="n")
    assert want == [0] and int(np.count_nonzero(o["flags"] & orc.F_FOUND)) > len(o["flags"]) // 2
    _check(stores["S1"], L, sel="n", pfs=(0,))


@pytest.mark.parametrize("L", [128, 150, 158])
def test_directed_reads(stores, L):
    """the runs that meet the word boundary and the read's end (their masks: test_gpu_single_node_reduce), as records"""
    for name in ("S1", "S3"):
        o, want = _check(stores[name], L, sel="directed")
        assert want[0] > len(o["flags"]) // 2


def test_127_values_few_counter_copies(stores):
    o, want = _check(stores["V127"], 150)
    assert want[0] > N // 4 and np.count_nonzero(o["table"][:, orc.C_READS]) > 60  # many rows take reads
    _check(stores["V127"], 158, pfs=(1,), max_read_tax_err=0.1, max_read_class_err=0.5)


def test_counters_in_hbm_defer_nothing(stores):
    """141 values: gs_match_kernel<false, ..> and its own deferred statistics; sn_info() says none, forced on or not"""
    o, _ = _check(stores["V141"], 150, lds=False)
    assert int(o["table"][:, orc.C_READS].sum()) > N // 4
