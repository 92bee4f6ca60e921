"""The reduce of a read with ONE distinct hit node in the FIXED loop of gs_match_kernel (counters in LDS).

Such a read books nothing on the way: its contigs are the runs of its hit masks, added up in scalar registers (count, sum of squares,
longest), and its statistics go out as one row of `sums`, one max key and one row of `dsums`.  Every other read takes the lane-parallel
booking.  Both must give what the oracle gives: integer table, class_vi and flags bit for bit, every cell of the double table within
tests/matchcheck.py's bound.  Every case is submitted with submit_fixed and again with an offsets array (the general loop, which
books every read by lanes); the two integer tables must be equal.

Stores (k = 31, 19 values: the LDS kernel):
  S1  every k-mer of the genomes; genus and root k-mers make some reads two-node, so both paths run in one batch;
  S2  a seeded pseudo-random half of S1's entries: reads from the genomes carry ragged hit masks (runs of one position, many runs
      per read, runs on both sides of position 63 / 64);
  S3  the species k-mers of S1 only: every read that hits is single-node (but for a handful whose substitutions make a k-mer of
      another species).
Reads (n = 4000 per case, read i of kind i % 14): from the genomes with 0, 1, 5 and 30 substitutions (kinds 0 .. 7), of these with an N
at base 0 (4), max - 2 (5), max - 1 (6) and L - 1 (7); background (8); directed reads, clean genome reads with substitutions placed so
that a hit run ends exactly at position 63 (9), starts exactly at 64 (10), covers 63 - 64 with both ends inside the words (11), ends at
max - 1 behind a gap (12), is the whole read (13).  A substitution at base b clears positions b - 30 .. b.
Needs an MI355X: run with -m gpu."""
import types

import numpy as np
import pytest

import genestrip_amd as ga
from genestrip_amd import synth
import matchcheck
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

N_READS = 4000
K = 31
N_KINDS = 14
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
DIRECTED = {9: (94,), 10: (63,), 11: (40, 110), 12: (50,), 13: ()}  # kind -> bases substituted in a clean genome read


def _substitute(rng, row, pos):
    code = np.searchsorted(ACGT, row[pos])
    row[pos] = ACGT[(code + rng.integers(1, 4, len(pos))) % 4]


def _reads(genomes, L, n, seed):
    """n reads of L bases back to back, read i of kind i % 14 (see the module docstring)"""
    mx = L - K + 1
    rng = np.random.default_rng(seed)
    g = rng.integers(0, genomes.shape[0], n)
    p = rng.integers(0, genomes.shape[1] - L + 1, n)
    seq = np.stack([genomes[g[i], p[i]:p[i] + L] for i in range(n)]).astype(np.uint8)
    kind = np.arange(n) % N_KINDS
    subs = (0, 1, 5, 30)
    for i in range(n):
        if kind[i] < 8:
            s = subs[(i // N_KINDS + kind[i]) % 4]
            if s:
                _substitute(rng, seq[i], rng.choice(L, size=s, replace=False))
        elif kind[i] in DIRECTED and DIRECTED[kind[i]]:
            _substitute(rng, seq[i], np.array(DIRECTED[kind[i]]))
    bg = kind == 8
    seq[bg] = ACGT[rng.integers(0, 4, (int(bg.sum()), L))]
    seq[kind == 4, 0] = ord("N")
    seq[kind == 5, mx - 2] = ord("N")
    seq[kind == 6, mx - 1] = ord("N")
    seq[kind == 7, L - 1] = ord("N")
    return seq.reshape(-1), (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))


def directed_mask(kind, mx):
    """the hit mask a directed read of this kind has on a store that holds every k-mer of the genomes"""
    m = np.ones(mx, dtype=bool)
    for b in DIRECTED[kind]:
        m[max(b - K + 1, 0):b + 1] = False
    return m


class _Store:
    def __init__(self, base, keep=None):
        kmers, vi = (base.kmers, base.value_idx) if keep is None else (base.kmers[keep], base.value_idx[keep])
        self.db = types.SimpleNamespace(k=K, kmers=kmers, value_idx=vi, n_values=base.n_values, parent_vi=base.parent_vi,
                                        genomes=base.genomes)
        self.odb = orc.DB(K, kmers, vi, base.n_values, base.parent_vi)
        self.store = ga.DeviceKMerStore(K, kmers, vi, base.n_values, base.parent_vi)
        self._reads = {}

    def reads(self, L):
        if L not in self._reads:
            self._reads[L] = _reads(self.db.genomes, L, N_READS, seed=1000 + L)
        return self._reads[L]

    def close(self):
        self.store.close()


@pytest.fixture(scope="module")
def base_db():
    db = synth.SynthDB(k=K, genera=3, species_per_genus=5, genome_len=20000)
    assert db.n_values == 19
    return db


@pytest.fixture(scope="module")
def stores(base_db):
    half = np.random.default_rng(5).random(len(base_db.kmers)) < 0.5
    s = dict(S1=_Store(base_db), S2=_Store(base_db, half), S3=_Store(base_db, np.isin(base_db.value_idx, base_db.species_vi)))
    yield s
    for x in s.values():
        x.close()


def _check(s, L, outputs=True, **cfg):
    """one length at one setting: fixed and offsets-array submit against the oracle and each other; returns the oracle's result"""
    n = N_READS
    seq, off = s.reads(L)
    what = f"L {L} outputs {outputs} {cfg}"
    o = matchcheck.oracle_batch(s.odb, seq, off, **cfg)
    ref = matchcheck.dtable_reference(o["terms"], s.db.n_values)
    m = ga.FastqKMerMatcher(s.store, ga.MatchConfig(**cfg))
    try:
        if outputs:
            cv_a, fl_a = m.match_reads(seq, off)
        else:
            cv_a = fl_a = None
            m.submit(seq, off, 0)
        t_a, d_a = m.finish()
        m.reset()
        cv_f, fl_f = (np.full(n, -7, dtype=np.int32), np.full(n, 0xee, dtype=np.uint8)) if outputs else (None, None)
        m.submit_fixed(seq, L, n, class_vi=cv_f, flags=fl_f)
        t_f, d_f = m.finish()
    finally:
        m.close()
    r_a = matchcheck.check_match(o, dict(table=t_a, dtable=d_a, class_vi=cv_a, flags=fl_a), what + " offsets array", ref=ref)
    r_f = matchcheck.check_match(o, dict(table=t_f, dtable=d_f, class_vi=cv_f, flags=fl_f), what + " fixed", ref=ref)
    print(f"{what}: counted {int(o['table'][:, orc.C_READS].sum())} of {n}, worst dtable ratio offsets {r_a:.3f} fixed {r_f:.3f}")
    assert np.array_equal(t_f, t_a), what + ": integer tables of the two submits differ"
    return o


def _is_what_it_claims(name, o):
    """from the oracle's own result: S1 has reads of more than one node, S2 more contigs than (read, node) pairs, S3 one node per read
    (but for a handful)"""
    t = o["table"]
    found = int(np.count_nonzero(o["flags"] & orc.F_FOUND))
    pairs = int(t[:, orc.C_READS_1KMER].sum())  # (read, tax id) pairs
    assert found > N_READS // 2
    if name == "S1":
        assert pairs > found
    if name == "S2":
        assert int(t[:, orc.C_CONTIGS].sum()) > pairs
        assert int(t[:, orc.C_CONTIGS].sum()) > 3 * found  # ragged: several runs per read
    if name == "S3":  # (a substituted k-mer that happens to be another species' own: a handful of reads in 4000)
        assert found <= pairs <= found + N_READS // 400


@pytest.mark.parametrize("L", [128, 143, 150, 158])
@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_lengths(stores, name, L):
    """98, 113, 120 and 128 positions (sub-round 1 holds 34, 49, 56 and 64 of them), ungated and with both gates at work"""
    o = _check(stores[name], L)
    _is_what_it_claims(name, o)
    assert 0 < int(o["table"][:, orc.C_READS].sum())
    _check(stores[name], L, max_read_tax_err=0.1, max_read_class_err=0.5)


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_settings(stores, name):
    """150 bases: a threshold above one, no classification, no unique counts, gates that let nothing but error-free reads through, no
    per-read outputs"""
    s = stores[name]
    _check(s, 150, threshold=3)
    o = _check(s, 150, classify=False)
    assert int(o["table"][:, orc.C_READS].sum()) == 0 and int(o["table"][:, orc.C_KMERS].sum()) > 0
    _check(s, 150, count_unique=False)
    _check(s, 150, max_read_tax_err=0.0, max_read_class_err=0.0)
    _check(s, 150, outputs=False)
    _check(s, 150, outputs=False, max_read_tax_err=0.1, max_read_class_err=0.5)


def test_general_loop_control(stores):
    """127 bases (97 positions): both submits take the general loop"""
    for name in ("S1", "S2", "S3"):
        _check(stores[name], 127)


@pytest.mark.parametrize("L", [128, 150, 158, 127])
def test_directed_reads_have_the_intended_masks(stores, L):
    """on S1 (every k-mer of the genomes) the oracle's segments of the directed reads are the runs they were built for"""
    s = stores["S1"]
    mx = L - K + 1
    seq, _ = s.reads(L)
    seq = seq.reshape(N_READS, L)
    for kind in DIRECTED:
        want = directed_mask(kind, mx)
        for i in range(kind, N_READS, N_KINDS * 40):
            got = np.concatenate([np.full(ln, code >= 0) for code, ln in s.odb.segments(seq[i].tobytes())])
            assert np.array_equal(got, want), (L, kind, i)
    # what the kinds are for: runs that end at 63, start at 64, cover 63 - 64 and end at max - 1, and one run over the whole read
    starts = {kind: np.flatnonzero(m & ~np.concatenate([[False], m[:-1]])).tolist() for kind, m in ((kd, directed_mask(kd, mx)) for kd in DIRECTED)}
    ends = {kind: np.flatnonzero(m & ~np.concatenate([m[1:], [False]])).tolist() for kind, m in ((kd, directed_mask(kd, mx)) for kd in DIRECTED)}
    assert 63 in ends[9] and 64 in starts[10] and mx - 1 in ends[12] and starts[13] == [0] and ends[13] == [mx - 1]
    assert starts[11][1] < 63 and ends[11][1] > 64 and ends[11][1] < mx - 1


@pytest.mark.parametrize("name", ["S1", "S3"])
def test_read_numbers_above_2_33_two_batches(stores, name):
    """first_read_no = 2^33 + 5, two batches of one run: the whole-read runs of the clean reads (kind 13: some 285 reads over 15
    species) tie on the longest contig, and MAX_CONTIG_READ_NO is the lowest read number among them"""
    s = stores[name]
    L, n, first = 150, N_READS, 2 ** 33 + 5
    mx = L - K + 1
    seq, off = s.reads(L)
    h = n // 2
    orun = orc.MatchRun(s.odb)
    m = ga.FastqKMerMatcher(s.store, ga.MatchConfig())
    ocv, ofl, terms, gcv, gfl = [], [], [], [], []
    try:
        for b in range(2):
            bs = seq[b * h * L:(b + 1) * h * L]
            cv, fl, te = orun.submit_terms(bs, off[:h + 1], first + b * h, threads=8)
            ocv.append(cv), ofl.append(fl), terms.append(te)
            cv_f, fl_f = np.full(h, -7, dtype=np.int32), np.full(h, 0xee, dtype=np.uint8)
            m.submit_fixed(bs, L, h, first_read_no=first + b * h, class_vi=cv_f, flags=fl_f)
            gcv.append(cv_f), gfl.append(fl_f)
        ot, od = orun.finish()
        gt, gd = m.finish()
    finally:
        m.close()
        orun.close()
    o = dict(table=ot, dtable=od, terms=np.concatenate(terms), class_vi=np.concatenate(ocv), flags=np.concatenate(ofl))
    longest = ot[:, orc.C_MAX_CONTIG_LEN] == mx
    assert longest.sum() >= 5  # rows whose longest contig is a whole read: ties among their clean reads
    assert np.all(ot[longest, orc.C_MAX_CONTIG_READ_NO] >= first) and np.all(ot[longest, orc.C_MAX_CONTIG_READ_NO] < first + n)
    matchcheck.check_match(o, dict(table=gt, dtable=gd, class_vi=np.concatenate(gcv), flags=np.concatenate(gfl)), f"{name} 2^33 + 5")
