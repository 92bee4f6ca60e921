"""The FIXED loop of gs_match_kernel without the minimizer gate (gs_probe_planes<.., NOGATE>, DESIGN 4 "Survivors skip the gate"):
every case runs with the gate dropped (GS_PF_GATE=0), kept (GS_PF_GATE=1) and through the CPU oracle.  Integer table (max keys and
unique counts are columns of it), class_vi and flags of every read are identical in all three; the double tables are within
matchcheck's bound of the exact sums and of each other (check_dtables_agree).  Every forced run asserts through gate_info() that
the batch went the way it was told.  A batch that cannot take the FIXED loop at all (GS_SN_DEFER=0 with counters in LDS: the general
loop) keeps its gate whatever GS_PF_GATE says, and the case asserts that.
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

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
VARS = ("GS_PF_GATE", "GS_PREFILTER", "GS_SN_DEFER")


def _windows(genomes, L, n, rng, sub_rate):
    """n windows of L bases from `genomes` (a 2-d array or a list of arrays) with `sub_rate` substitutions per base"""
    seq = np.empty((n, L), dtype=np.uint8)
    for i in range(n):
        g = genomes[int(rng.integers(0, len(genomes)))]
        p = int(rng.integers(0, len(g) - L + 1))
        seq[i] = g[p:p + L]
    sub = rng.random((n, L)) < sub_rate
    seq[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    return seq


def _prefix_reads(genomes, L, n, rng, S=None, k=31):
    """reads whose first 15 bases come from a genome and whose other bases are uniform random; with S (the store's canonical
    15-mers, prefilter.lmer_set) only reads whose sample 0 is in S: they pass the prefilter and hit nothing"""
    seq = _windows(genomes, L, 3 * n if S is not None else n, rng, 0.0)
    seq[:, 15:] = ACGT[rng.integers(0, 4, (len(seq), L - 15))]
    if S is not None:
        canon, bad = pf.sample_codes(seq, L, k)
        seq = seq[np.isin(canon[:, 0], S) & ~bad[:, 0]][:n]
        assert len(seq) == n
    return seq


def _spoiled(genomes, L, n, rng):
    """genome reads with one N (rows 0, 1, 2 of every six) or a lower-case stretch (rows 3, 4, 5) that touches only the first
    window, a middle window, only the last window: act = live & ~invalid at both ends of both sub-rounds"""
    seq = _windows(genomes, L, n, rng, 0.01)
    for r in range(n):
        kind = r % 6
        if kind < 3:
            seq[r, (0, L // 2, L - 1)[kind]] = ord("N")
        else:
            a = (0, L // 2, L - 6)[kind - 3]
            seq[r, a:a + 6] |= 0x20
    return seq


def _mixed(genomes, L, n, seed, S=None):
    """n reads, an eighth each (interleaved, so that every batch size holds every kind): genome windows with 1 % and with 5 %
    substitutions (x2 each), prefix reads, spoiled reads, uniform background (x2)"""
    rng = np.random.default_rng(seed)
    m = (n + 7) // 8
    kinds = [_windows(genomes, L, m, rng, 0.01), _windows(genomes, L, m, rng, 0.05), _prefix_reads(genomes, L, m, rng, S),
             _spoiled(genomes, L, m, rng), ACGT[rng.integers(0, 4, (m, L))], _windows(genomes, L, m, rng, 0.05),
             _windows(genomes, L, m, rng, 0.01), ACGT[rng.integers(0, 4, (m, L))]]
    return np.ascontiguousarray(np.stack(kinds, axis=1).reshape(-1, L)[:n])


class _Store:
    def __init__(self, k, kmers, vidx, n_values, parent_vi):
        self.k = k
        self.odb = orc.DB(k, kmers, vidx, n_values, parent_vi)
        self.dev = ga.DeviceKMerStore(k, kmers, vidx, n_values, parent_vi)

    def close(self):
        self.dev.close()


def _device(store, gate, batches, L, prefilter=None, defer=None, **cfg):
    """one run over `batches` = [(seq, n, first)], begun under GS_PF_GATE = gate, GS_PREFILTER = prefilter, GS_SN_DEFER = defer (None:
    unset; the library reads them when a run begins); the result, and gate_info() and prefilter_info() behind every batch"""
    before = {v: os.environ.pop(v, None) for v in VARS}
    for v, x in zip(VARS, (gate, prefilter, defer)):
        if x is not None:
            os.environ[v] = str(x)
    try:
        m = ga.FastqKMerMatcher(store.dev, ga.MatchConfig(**cfg))
    finally:
        for v in VARS:
            os.environ.pop(v, None)
            if before[v] is not None:
                os.environ[v] = before[v]
    try:
        cvs, fls, gates, pfs = [], [], [], []
        for seq, n, first in batches:
            cv = np.full(n, -7, dtype=np.int32)
            fl = np.full(n, 0xee, dtype=np.uint8)
            m.submit_fixed(np.ascontiguousarray(seq).reshape(-1), L, n, first, class_vi=cv, flags=fl)
            gates.append(m.gate_info())
            pfs.append(m.prefilter_info())
            cvs.append(cv)
            fls.append(fl)
        t, d = m.finish()
        res = dict(table=t, dtable=d, class_vi=np.concatenate(cvs), flags=np.concatenate(fls))
        if cfg.get("max_kmer_res_counts"):
            res["max_counts"] = m.max_counts()
    finally:
        m.close()
    return res, gates, pfs


def _oracle(store, seq, L, n, first=0, **cfg):
    seq = np.ascontiguousarray(seq).reshape(-1, L)[:n]
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    return matchcheck.oracle_batch(store.odb, seq.reshape(-1), off, first_read_no=first, max_counts=bool(cfg.get("max_kmer_res_counts")), **cfg)


def _check(store, batches, L, what, o, prefilter=None, defer=None, can=True, **cfg):
    """both forced runs over `batches` against the oracle result o and against each other; can: the batches can take the FIXED loop"""
    off, g_off, p_off = _device(store, 0, batches, L, prefilter, defer, **cfg)
    on, g_on, p_on = _device(store, 1, batches, L, prefilter, defer, **cfg)
    matchcheck.check_match(o, off, what + ", gate dropped")
    matchcheck.check_match(o, on, what + ", gate kept")
    assert np.array_equal(off["table"], on["table"]), what
    assert np.array_equal(off["class_vi"], on["class_vi"]) and np.array_equal(off["flags"], on["flags"]), what
    matchcheck.check_dtables_agree(off["dtable"], on["dtable"], on["table"][:, orc.C_READS], what + ": double tables dropped / kept")
    if "max_counts" in off:
        assert np.array_equal(off["max_counts"], on["max_counts"]), what
    assert all(g["gateless"] == can for g in g_off), (what, g_off)
    assert not any(g["gateless"] for g in g_on), (what, g_on)
    assert all(0.0 <= g["predicted_pass"] <= 1.0 for g in g_off + g_on) if can else all(g["predicted_pass"] == -1.0 for g in g_off + g_on)
    for a, b in zip(p_off, p_on):  # the gate decides nothing about the prefilter
        assert a == b, (what, a, b)
    return off, p_off


@pytest.fixture(scope="module")
def db31():
    return synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)


@pytest.fixture(scope="module")
def st31(db31):
    s = _Store(31, db31.kmers, db31.value_idx, db31.n_values, db31.parent_vi)
    yield s
    s.close()


@pytest.fixture(scope="module")
def S31(db31):
    return pf.lmer_set(db31.kmers, 31)


@pytest.fixture(scope="module")
def mix150(db31, S31):
    return _mixed(db31.genomes, 150, 4096, seed=150, S=S31)


@pytest.fixture(scope="module")
def oracle2000(st31, mix150):
    """the 2 000 reads the configuration cases share, through the oracle once"""
    return _oracle(st31, mix150, 150, 2000)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_batch_sizes(st31, mix150, n):
    o = _oracle(st31, mix150, 150, n)
    if n >= 63:
        assert (o["flags"] & orc.F_FOUND).any() and not (o["flags"] & orc.F_FOUND).all()
    _check(st31, [(mix150[:n], n, 0)], 150, f"{n} reads", o)


@pytest.mark.parametrize("L", [128, 150, 158])
def test_lengths(st31, db31, S31, L):
    """65, 120 and 128 positions at k = 31 would be L = 95, 150, 158; the FIXED loop starts at L = 128 (98 positions): the shortest
    read it takes, a read in the middle, and the longest (sub-round 1 full)"""
    seq = _mixed(db31.genomes, L, 1500, seed=L, S=S31)
    _check(st31, [(seq, 1500, 0)], L, f"L {L}", _oracle(st31, seq, L, 1500))


@pytest.mark.parametrize("defer", [1, 0], ids=["defer", "no_defer"])
@pytest.mark.parametrize("prefilter", [0, 1, None], ids=["pf_off", "pf_on", "pf_rules"])
def test_prefilter_and_defer_modes(st31, mix150, oracle2000, prefilter, defer):
    """GS_SN_DEFER=0 sends the batch through the general loop (counters in LDS): it cannot drop the gate, and says so"""
    _, pfs = _check(st31, [(mix150[:2000], 2000, 0)], 150, f"prefilter {prefilter} defer {defer}", oracle2000, prefilter=prefilter,
                    defer=defer, can=defer == 1)
    assert (pfs[0]["survivors"] == -1) == (prefilter == 0)


def test_only_background(st31):
    rng = np.random.default_rng(5)
    seq = ACGT[rng.integers(0, 4, (3000, 150))]
    o = _oracle(st31, seq, 150, 3000)
    assert not np.any(o["table"][:, orc.C_READS])
    _, pfs = _check(st31, [(seq, 3000, 0)], 150, "background only", o, prefilter=1)
    assert 0 <= pfs[0]["survivors"] <= 300


def test_prefix_reads_probe_every_lane(st31, db31, S31):
    """every read passes the prefilter at sample 0 and hits nothing: with the gate dropped every lane loads its record lines"""
    seq = _prefix_reads(db31.genomes, 150, 1000, np.random.default_rng(9), S=S31)
    o = _oracle(st31, seq, 150, 1000)
    _, pfs = _check(st31, [(seq, 1000, 0)], 150, "prefix reads", o, prefilter=1)
    assert pfs[0]["survivors"] == 1000
    assert int((o["flags"] & orc.F_FOUND).sum()) <= 50  # (a random tail of 135 bases seldom completes a stored 31-mer)


@pytest.mark.parametrize("unique", [True, False], ids=["unique", "no_unique"])
def test_marks_and_hit_counters_do_not_move(st31, mix150, unique):
    """unique marks and per-k-mer hit counters are taken only on a hit: a lane the gate would have stopped must leave none"""
    cfg = dict(count_unique=unique, threshold=2)
    if unique:  # (hit counters exist only next to the unique marks)
        cfg["max_kmer_res_counts"] = 5
    o = _oracle(st31, mix150, 150, 2000, first=2 ** 33 + 5, **cfg)
    assert not unique or np.any(o["max_counts"])
    off, _ = _check(st31, [(mix150[:2000], 2000, 2 ** 33 + 5)], 150, f"unique {unique}, max counts", o, **cfg)
    t = off["table"]
    assert np.all(t[:, orc.C_UNIQUE_KMERS] >= 0) if unique else np.all(t[:, orc.C_UNIQUE_KMERS] == -1)
    assert not unique or np.any(t[:, orc.C_UNIQUE_KMERS] > 0)


def test_two_batches_in_one_run(st31, mix150):
    o = _oracle(st31, mix150, 150, 4096)
    batches = [(mix150[:2049], 2049, 0), (mix150[2049:], 2047, 2049)]
    _check(st31, batches, 150, "two batches", o)
    _check(st31, batches, 150, "two batches, prefilter on", o, prefilter=1)


_GLOBAL_STATS = """
import numpy as np
import test_gpu_gateless as t
import prefilter as pf
from genestrip_amd import synth
db = synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)
s = t._Store(31, db.kmers, db.value_idx, db.n_values, db.parent_vi)
seq = t._mixed(db.genomes, 150, 4096, seed=150, S=pf.lmer_set(db.kmers, 31))
t._check(s, [(seq, 4096, 0)], 150, "global statistics", t._oracle(s, seq, 150, 4096))
s.close()
print("global statistics ok")
"""


def test_global_statistics_instantiation():
    """GS_FORCE_GLOBAL_STATS=1: the loop is one body of code, so gs_match_kernel<false, ..> (counters in global memory, deferred
    records, seen bits aggregated per record line) has the gate-less variant too.  The launchers read the variable once per process,
    so the case runs in a process of its own"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, GS_FORCE_GLOBAL_STATS="1", PYTHONPATH=os.pathsep.join([here, os.path.dirname(here)]))
    r = subprocess.run([sys.executable, "-s", "-c", _GLOBAL_STATS], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "global statistics ok" in r.stdout, (r.stdout[-800:], r.stderr[-3000:])


def test_skewed_store_with_overflow_table():
    """low-complexity islands give minimizers with three and more windows: record lines carry the `more` bit and the overflow table is
    populated -- the only place where a lane without the gate walks the table for a k-mer that is not stored"""
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
        assert info.n_in_records < info.n_stored  # the overflow table is not empty
        reads = _mixed(sdb.genomes, 150, 4096, seed=77)
        o = _oracle(s, reads, 150, 4096, count_unique=True, max_kmer_res_counts=3)
        assert (o["flags"] & orc.F_FOUND).any()
        _check(s, [(reads, 4096, 0)], 150, "skewed store", o, count_unique=True, max_kmer_res_counts=3)
        _check(s, [(reads, 4096, 0)], 150, "skewed store, prefilter on", o, prefilter=1, count_unique=True, max_kmer_res_counts=3)
    finally:
        s.close()


def test_rule_is_a_pure_function():
    samples = len(pf.sample_positions(150, 31))
    bench = int(2.0 ** 29 * (1.0 - (1.0 - 0.028) ** (1.0 / samples)))  # the |S| at which the bench store's 0.028 is predicted
    for n_lmers in (0, 1000, bench):
        g, p = ga.gate_rule(n_lmers, samples)
        assert g and p == pytest.approx(1.0 - (1.0 - n_lmers / 2.0 ** 29) ** samples, abs=1e-12)
    assert ga.gate_rule(bench, samples)[1] == pytest.approx(0.028, abs=0.0001)
    # a store dense enough that nearly every random read passes keeps its gate, and so does one whose 15-mers were never counted
    assert ga.gate_rule(2 ** 28, samples) == (False, pytest.approx(1.0 - 0.5 ** samples))
    assert ga.gate_rule(-1, samples) == (False, 1.0)
    # monotonic in |S|: one switch from gate-less to gated
    flags = [ga.gate_rule(n, samples)[0] for n in np.linspace(0, 2 ** 28, 200).astype(np.int64)]
    assert flags[0] and not flags[-1] and sum(a != b for a, b in zip(flags, flags[1:])) == 1
    # GS_PF_GATE decides whatever the store
    assert ga.gate_rule(2 ** 28, samples, 0)[0] and not ga.gate_rule(1000, samples, 1)[0]


def test_rule_on_the_device(st31, mix150, oracle2000):
    """under unset variables the small store goes through the prefilter and drops the gate, with the probability the rule gives for
    its |S|; with the prefilter forced off nothing says that the reads are from the store, and the gate stays"""
    res, gates, pfs = _device(st31, None, [(mix150[:2000], 2000, 0)], 150)
    matchcheck.check_match(oracle2000, res, "under the rules")
    want = ga.gate_rule(pfs[0]["n_lmers"], len(pf.sample_positions(150, 31)))
    assert pfs[0]["survivors"] >= 0 and want[0]
    assert gates[0] == {"gateless": True, "predicted_pass": want[1]}
    res, gates, pfs = _device(st31, None, [(mix150[:2000], 2000, 0)], 150, prefilter=0)
    matchcheck.check_match(oracle2000, res, "under the gate rule, prefilter off")
    assert pfs[0]["survivors"] == -1 and not gates[0]["gateless"]


def test_paused_batches_stay_gateless(st31, db31):
    """a stream of genome reads: the first batch goes through the prefilter, nearly all of it survives, the feedback rule sends the
    next batches past the prefilter -- and, by the same evidence, past the gate; results equal the oracle across the switch"""
    rng = np.random.default_rng(31)
    a, b = _windows(db31.genomes, 150, 2000, rng, 0.01), _windows(db31.genomes, 150, 2000, rng, 0.05)
    o = _oracle(st31, np.concatenate([a, b]), 150, 4000)
    res, gates, pfs = _device(st31, None, [(a, 2000, 0), (b, 2000, 2000)], 150)
    assert pfs[0]["survivors"] > 1700 and pfs[1]["survivors"] == -1, pfs
    assert gates[0]["gateless"] and gates[1]["gateless"], gates
    matchcheck.check_match(o, res, "paused batch")
    kept, gates, _ = _device(st31, 1, [(a, 2000, 0), (b, 2000, 2000)], 150)
    assert not gates[0]["gateless"] and not gates[1]["gateless"]
    matchcheck.check_match(o, kept, "paused batch, gate kept")
    assert np.array_equal(res["table"], kept["table"])
