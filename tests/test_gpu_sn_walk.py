"""The FIXED loop of gs_match_kernel (counters in LDS) only looks k-mers up: every read leaves the wave as a record.  A read without
a non-CGAT byte whose hit k-mers carry one tax id is a GsSnRec (tests/test_gpu_sn_defer.py); a read of several tax ids or with a byte
that is no upper-case CGAT letter leaves as the node of every position, gs_sn_reduce_kernel lists it and gs_sn_walk_kernel walks it
in one lane (gs_sn_walk, genestrip_amd/csrc/gs_snrec.h; tests/test_snwalk_steps_cpu.py holds the walk itself to a restatement).

Stores of 20 and 127 values (k = 31, counters in LDS; 127: four counter copies per workgroup):
  K20, K127  synth.SkewedDB, built by the oracle's DbBuild: 21 .. 29 % of every genome is shared with its genus, 5 % with every
             genome, two strains copy a species, so reads of two and three tax ids are common.  Reads: synth.skewed_reads "ragged"
             (every genome, both strands, substitutions, 2 % with a run of N, 2 % with a lower-case stretch), those of L bases or
             more cut to L, every 8th read replaced by background and every 64th by background with an N;
  Y20, Y127  synth.SynthDB with reads of synth.reads_device (the benchmark's stream, clean genome windows).
Every case runs with GS_SN_DEFER=1 and =0 (off: the general loop books every read itself) and with GS_PREFILTER=0 (slot = read number)
and =1 (slot = index into the survivor list) and holds the integer table, class_vi and flags of each run to the oracle bit for bit
and the double table within tests/matchcheck.py's bound.  sn_info() must report exactly the reads of one tax id and the reads that
left as rows, both counted here from the oracle's segments; behind the prefilter a read with a bad byte and no hit may be dropped
before it is a row, so there the rows lie between the rows with a hit and all rows.
Needs an MI355X: run with -m gpu."""
import os

import numpy as np
import pytest

import genestrip_amd as ga
from genestrip_amd import synth
import matchcheck
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

K = 31
N = 4096
CGAT = np.zeros(256, dtype=bool)
CGAT[list(b"ACGT")] = True


class _Env:
    """environment variables the library reads when a run begins"""

    def __init__(self, **kv):
        self.kv = kv

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


class _Store:
    def __init__(self, kmers, vi, n_values, parent_vi):
        self.n_values = n_values
        self.odb = orc.DB(K, kmers, vi, n_values, parent_vi)
        self.store = ga.DeviceKMerStore(K, kmers, vi, n_values, parent_vi)
        self.rows = {}   # L -> reads [n][L]
        self.kinds = {}  # L -> per read: 0 no hit and clean, 1 one tax id and clean, 2 a row with a hit, 3 a row without one
        self.cache = {}

    def close(self):
        self.store.close()


def _skewed(n_values, seed):
    db = synth.SkewedDB(genera=3, species_per_genus=4, genome_len=60_000, strains=2, dominant_len=1000, n_values=n_values, seed=seed)
    assert db.n_values == n_values
    seq, off, nvi = db.regions()
    b = orc.DbBuild(K, db.n_values, db.parent_vi)
    b.fill(seq, off, nvi)
    b.optimize()
    b.update(seq, off, nvi)
    kmers, vidx = b.fetch()
    b.close()
    s = _Store(kmers, vidx, db.n_values, db.parent_vi)
    rseq, roff, _ = synth.skewed_reads(db, 48_000, "ragged", seed=seed, sub_rate=0.004)
    roff = roff.astype(np.int64)
    length = np.diff(roff)
    for L in (128, 150, 158):
        idx = np.flatnonzero(length >= L)[:N]
        assert len(idx) == N
        rows = np.stack([rseq[roff[i]:roff[i] + L] for i in idx])
        # every 8th read (from the fourth on) is background, and every 64th of these has an N: a row without a hit
        rng = np.random.default_rng(seed + L)
        bg = np.arange(3, N, 8)
        rows[bg] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (len(bg), L))]
        rows[bg[::8], rng.integers(0, L, len(bg[::8]))] = ord("N")
        s.rows[L] = rows
    return s


def _synth(genera, species, seed):
    import torch
    db = synth.SynthDB(k=K, genera=genera, species_per_genus=species, genome_len=8000, seed=seed)
    s = _Store(db.kmers, db.value_idx, db.n_values, db.parent_vi)
    gen = torch.from_numpy(db.genomes).cuda()
    for L in (128, 150, 158):
        dseq = torch.empty(N * L, dtype=torch.uint8, device="cuda")
        doff = torch.empty(N + 1, dtype=torch.int64, device="cuda")
        synth.reads_device(gen, db.genomes.shape[0], db.genomes.shape[1], N, dseq, doff, read_len=L, seed=4242 + L)
        s.rows[L] = dseq.cpu().numpy().reshape(N, L)
    return s


@pytest.fixture(scope="module")
def stores():
    s = dict(K20=_skewed(20, 31), K127=_skewed(127, 32), Y20=_synth(1, 18, 7), Y127=_synth(6, 20, 9))
    assert [s[x].n_values for x in ("K20", "K127", "Y20", "Y127")] == [20, 127, 20, 127]
    yield s
    for x in s.values():
        x.close()


def _kinds(s, L):
    if L not in s.kinds:
        kind = np.zeros(len(s.rows[L]), dtype=np.int8)
        for i, row in enumerate(s.rows[L]):
            nodes = {code for code, _ in s.odb.segments(row.tobytes()) if code >= 0}
            if CGAT[row].all():
                kind[i] = 0 if not nodes else (1 if len(nodes) == 1 else 2)
            else:
                kind[i] = 2 if nodes else 3
        s.kinds[L] = kind
    return s.kinds[L]


def _oracle(s, L, sel, batches, first, cfg):
    key = (L, sel.tobytes(), tuple(batches), first, tuple(sorted(cfg.items())))
    if key not in s.cache:
        rows = s.rows[L][sel]
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
        s.cache[key] = (o, matchcheck.dtable_reference(o["terms"], s.n_values))
    return s.cache[key]


def _device(s, L, sel, batches, first, defer, pf, cfg):
    rows = s.rows[L][sel]
    with _Env(GS_SN_DEFER=defer, GS_PREFILTER=pf):
        m = ga.FastqKMerMatcher(s.store, ga.MatchConfig(**cfg))
    cvs, fls, infos, no = [], [], [], first
    try:
        for a, b in batches:
            part = np.ascontiguousarray(rows[a:b])
            cv = np.full(len(part), -7, dtype=np.int32)
            fl = np.full(len(part), 0xee, dtype=np.uint8)
            m.submit_fixed(part.reshape(-1), L, len(part), first_read_no=no, class_vi=cv, flags=fl)
            infos.append((m.sn_info(), m.prefilter_info()))
            cvs.append(cv), fls.append(fl)
            no += len(part)
        t, d = m.finish()
    finally:
        m.close()
    return dict(table=t, dtable=d, class_vi=np.concatenate(cvs), flags=np.concatenate(fls)), infos


def _check(s, L, sel=None, batches=None, first=0, pfs=(0, 1), **cfg):
    """one case under GS_SN_DEFER = 1 and 0 and every GS_PREFILTER of pfs; returns the kinds of the selected reads"""
    kind = _kinds(s, L)
    sel = np.ones(len(kind), dtype=bool) if sel is None else sel
    kind = kind[sel]
    batches = [(0, len(kind))] if batches is None else batches
    o, ref = _oracle(s, L, sel, batches, first, cfg)
    for pf in pfs:
        for defer in (1, 0):
            what = f"{s.n_values} values L {L} batches {batches} prefilter {pf} defer {defer} {cfg}"
            g, infos = _device(s, L, sel, batches, first, defer, pf, cfg)
            ratio = matchcheck.check_match(o, g, what, ref=ref)
            print(f"{what}: {[i for i, _ in infos]}, kinds {np.bincount(kind, minlength=4).tolist()}, worst dtable ratio {ratio:.3f}")
            for (sn, pi), (a, b) in zip(infos, batches):
                assert (pi["survivors"] >= 0) == bool(pf), (what, pi)
                one, hit_rows, all_rows = (int(np.count_nonzero(kind[a:b] == 1)), int(np.count_nonzero(kind[a:b] == 2)),
                                           int(np.count_nonzero(kind[a:b] >= 2)))
                if not defer:
                    assert not sn["deferred"] and sn["booked"] == 0 and sn["rows"] == 0, (what, sn)
                else:
                    assert sn["deferred"] and sn["booked"] == one, (what, sn, one)
                    assert sn["rows"] == all_rows if not pf else hit_rows <= sn["rows"] <= all_rows, (what, sn, hit_rows, all_rows)
    return kind


def _window(kind, n):
    """n reads in a row that start at the first read of several tax ids"""
    start = int(np.flatnonzero(kind == 2)[0])
    start = min(start, len(kind) - n)
    sel = np.zeros(len(kind), dtype=bool)
    sel[start:start + n] = True
    return sel


@pytest.mark.parametrize("L", [128, 150, 158])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_batch_sizes_and_lengths(stores, L, n):
    """98, 120 and 128 positions; fewer rows than a wave has lanes, as many, one more, and sixteen workgroups of them"""
    s = stores["K20"]
    kind = _check(s, L, sel=_window(_kinds(s, L), n))
    assert np.count_nonzero(kind == 2) >= 1
    if n == 4096:  # reads of several tax ids are common, and the N runs and lower-case stretches are there
        assert np.count_nonzero(kind == 2) > n // 10 and np.count_nonzero(kind == 1) > n // 8
        assert np.count_nonzero(kind == 3) >= 32 and np.count_nonzero(kind == 0) > n // 10
        assert np.count_nonzero(~CGAT[s.rows[L]].all(axis=1) & (kind == 2)) >= 32  # N runs and lower-case stretches in reads that hit


@pytest.mark.parametrize("name", ["K127", "Y20", "Y127"])
def test_other_stores(stores, name):
    """127 values (four counter copies), and the benchmark's reads on stores of both sizes"""
    s = stores[name]
    for L in (128, 150, 158) if name == "K127" else (150,):
        kind = _check(s, L)
        assert np.count_nonzero(kind == 2) >= (N // 10 if name == "K127" else 1) and np.count_nonzero(kind == 1) > N // 8


@pytest.mark.parametrize("name", ["K20", "K127"])
def test_every_read_a_row_and_none(stores, name):
    s = stores[name]
    kind = _kinds(s, 150)
    only = _check(s, 150, sel=kind >= 2)
    assert len(only) > N // 10 and np.all(only >= 2)
    none = _check(s, 150, sel=kind < 2)
    assert len(none) > N // 8 and np.all(none < 2)


def test_two_batches_second_smaller(stores):
    """one run, 2500 reads and then 1596: behind the second batch's records and rows lie the first one's"""
    for name in ("K20", "K127"):
        kind = _check(stores[name], 150, batches=[(0, 2500), (2500, N)], first=2 ** 33 + 5)
        assert np.count_nonzero(kind[2500:] == 2) > 100


@pytest.mark.parametrize("name", ["K20", "K127"])
def test_settings(stores, name):
    """one path and two, thresholds 3 and above any count, both gates, no classification"""
    s = stores[name]
    _check(s, 150, pfs=(1,), threshold=3, max_paths=1, max_read_tax_err=0.1, max_read_class_err=0.3)
    _check(s, 158, pfs=(0,), threshold=3, max_paths=2)
    _check(s, 128, pfs=(0,), threshold=200)
    _check(s, 150, pfs=(0,), classify=False)
    _check(s, 150, pfs=(1,), max_read_tax_err=0.0, max_read_class_err=0.0)
