"""The work of a match step around the match kernel: gs_match_finish's one sweep over the store (compact bitmap and unique counts
together), the one packed copy of the result, the launches a batch of short reads of one length no longer makes, and the bitmap
that gs_match_reset no longer clears.  Every case holds the whole table, unique column included, to the CPU oracle.
Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
from genestrip_amd import synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

UNIQ_LDS = 8192  # GS_UNIQ_LDS of gs_seen.hip: value indices counted in LDS
N = 2000         # reads per batch, at most


class _Store:
    """the arrays of a store, its oracle copy and (lazily) its device copy"""

    def __init__(self, k, kmers, vidx, n_values, parent, genomes):
        self.k, self.kmers, self.vidx, self.n_values, self.parent, self.genomes = k, kmers, vidx, n_values, parent, genomes
        self.odb = orc.DB(k, kmers, vidx, n_values, parent)
        self._dev = None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = ga.DeviceKMerStore(self.k, self.kmers, self.vidx, self.n_values, self.parent)
        return self._dev

    def close(self):
        if self._dev is not None:
            self._dev.close()


def _of_synth(k):
    db = synth.SynthDB(k=k)
    return _Store(k, db.kmers, db.value_idx, db.n_values, db.parent_vi, db.genomes)


def _of_arrays(n_values, seed):
    """a few thousand k-mers of one random sequence, every one its own value index drawn from the whole range 1 .. n_values - 1 (the
    two largest indices among them), all children of the root"""
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 6000)
    kmers = np.unique(orc.canonical_kmers(genome.tobytes().decode(), 31)).astype(np.int64)
    vidx = rng.integers(1, n_values, len(kmers)).astype(np.int32)
    vidx[:4] = [n_values - 1, n_values - 2, 1, n_values - 1]
    parent = np.zeros(n_values, dtype=np.int32)
    parent[0] = -1
    return _Store(31, kmers, vidx, n_values, parent, genome[None, :])


@pytest.fixture(scope="module")
def stores():
    made = {}

    def get(name):
        if name not in made:
            made[name] = {"rec31": lambda: _of_synth(31), "table16": lambda: _of_synth(16),
                          "nv8193": lambda: _of_arrays(UNIQ_LDS + 1, 5), "nv8192": lambda: _of_arrays(UNIQ_LDS, 6)}[name]()
        return made[name]

    yield get
    for s in made.values():
        s.close()


def _reads(genomes, n, length, seed, rows=None):
    """n reads of one length from random places of the genomes `rows` (default: all): (seq, offsets)"""
    rng = np.random.default_rng(seed)
    rows = np.arange(genomes.shape[0]) if rows is None else np.asarray(rows)
    g = rows[rng.integers(0, len(rows), n)]
    p = rng.integers(0, genomes.shape[1] - length + 1, n)
    seq = genomes[g[:, None], p[:, None] + np.arange(length)[None, :]].reshape(-1)
    return np.ascontiguousarray(seq, dtype=np.uint8), (np.arange(n + 1, dtype=np.uint64) * np.uint64(length))


def _mixed(genomes, lengths, per_length, seed):
    """reads of several lengths, interleaved: (seq, offsets)"""
    parts = [_reads(genomes, per_length, L, seed + L)[0].reshape(per_length, L) for L in lengths]
    rows = [parts[i][j] for j in range(per_length) for i in range(len(lengths))]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    return np.concatenate(rows), off


def _submit(m, batch, first):
    """batch: (seq, offsets) -- as reads of one length (gs_match_submit_fixed) when `offsets` is an int, the read length"""
    seq, off = batch
    if isinstance(off, (int, np.integer)):
        m.submit_fixed(seq, int(off), len(seq) // int(off), first_read_no=first)
        m.sync()
        return len(seq) // int(off)
    m.match_reads(seq, off, first)
    return len(off) - 1


def _offsets(batch):
    seq, off = batch
    if isinstance(off, (int, np.integer)):
        return np.arange(len(seq) // int(off) + 1, dtype=np.uint64) * np.uint64(off)
    return off


class _Oracle:
    """an oracle run fed batch by batch: result() is what check_match takes, over all reads so far"""

    def __init__(self, store, **cfg):
        self.run, self.terms = orc.MatchRun(store.odb, **cfg), []

    def submit(self, batch, first):
        _, _, te = self.run.submit_terms(batch[0], _offsets(batch), first)
        self.terms.append(te)

    def result(self):
        t, d = self.run.finish()
        return dict(table=t, dtable=d, terms=np.concatenate(self.terms))


def _run(store, batches, **cfg):
    """the batches through one device run and one oracle run: (matcher, oracle result)"""
    m = ga.FastqKMerMatcher(store.dev, ga.MatchConfig(**cfg))
    o = _Oracle(store, **cfg)
    first = 0
    for b in batches:
        o.submit(b, first)
        first += _submit(m, b, first)
    return m, o


def _check(o, m, what):
    t, d = m.finish()
    matchcheck.check_match(o.result() if isinstance(o, _Oracle) else o, dict(table=t, dtable=d), what)
    return t, d


@pytest.mark.parametrize("name", ["rec31", "table16", "nv8193", "nv8192"])
def test_sweep_paths(stores, name):
    """records and table slots, table slots alone, and the switch from LDS counters to global atomics"""
    s = stores(name)
    info = s.dev.info
    assert (info.rec_bytes > 0) == (name != "table16") and info.n_values == s.n_values
    fixed = (_reads(s.genomes, N, 150, 1)[0], 150)
    m, o = _run(s, [fixed, _reads(s.genomes, 500, 140, 2)])
    t, _ = _check(o, m, name)
    uniq = t[:, ga.COLS.index("unique kmers")]
    assert uniq.sum() > 1000
    if name.startswith("nv"):
        assert uniq[s.n_values - 1] > 0 and uniq[s.n_values - 2] > 0 and np.count_nonzero(uniq) > 500
    m.close()


def test_finish_twice_and_more_reads(stores):
    s = stores("rec31")
    a, b = (_reads(s.genomes, N, 150, 3)[0], 150), (_reads(s.genomes, N, 150, 4)[0], 150)
    m, o = _run(s, [a])
    t1, d1 = _check(o, m, "first finish")
    t2, d2 = m.finish()
    assert np.array_equal(t1, t2) and np.array_equal(d1, d2)
    o.submit(b, N)
    _submit(m, b, N)
    _check(o, m, "finish after more reads")
    m.close()


def test_reset_leaves_no_bitmap_bits(stores):
    """batch A touches one half of the store, batch B after a reset the other: bits of A that stayed in the compact bitmap
    (gs_match_reset does not clear it) would count for B"""
    s = stores("rec31")
    a = (_reads(s.genomes, N, 150, 5, rows=range(0, 10))[0], 150)
    b = (_reads(s.genomes, N, 150, 6, rows=range(10, 20))[0], 150)
    m, o = _run(s, [a])
    ta, _ = _check(o, m, "batch A")
    m.reset()
    ob = _Oracle(s)
    ob.submit(b, 0)
    _submit(m, b, 0)
    tb, _ = _check(ob, m, "batch B after reset")
    u = ga.COLS.index("unique kmers")
    assert ta[:, u].sum() > 0 and tb[:, u].sum() > 0 and not np.array_equal(ta[:, u], tb[:, u])
    # ... and through the path that reads the bitmap without an extract before it: the OR of a part into it, right after a reset
    m.reset()
    _submit(m, a, 0)
    words = m.device_state()["bitmap_words"]
    empty = ga.FastqKMerMatcher(s.dev, ga.MatchConfig(count_unique=False))  # (its bitmap: zero from the start, never written)
    part = empty.device_state()
    assert part["bitmap_words"] == words
    m.reset()
    m.or_bitmap(part["bitmap"], 1)  # an empty part into a reset run: no k-mer is seen
    t, _ = m.finish()
    assert t[:, u].sum() == 0
    empty.close()
    m.close()


@pytest.mark.parametrize("name", ["rec31", "table16"])
def test_merged_bitmap_path_agrees(stores, name):
    """the counts from a merged bitmap (gs_rec_unique_count_kernel / gs_unique_count_kernel) against the fused sweep's"""
    s = stores(name)
    m, o = _run(s, [(_reads(s.genomes, N, 150, 7)[0], 150)])
    ores = o.result()
    t1, d1 = _check(ores, m, "fused sweep")
    st = m.device_state()
    m.or_bitmap(st["bitmap"], 1)
    t2, d2 = _check(ores, m, "merged bitmap")
    assert np.array_equal(t1, t2) and np.array_equal(d1, d2)
    m.close()


@pytest.mark.parametrize("order", ["fixed-mixed-fixed", "mixed-fixed-mixed"])
def test_queues_across_batches(stores, order):
    """a batch that launches no queue kernel and leaves the queue counters alone, between batches that fill all three queues"""
    s = stores("rec31")
    fixed = [(_reads(s.genomes, N, 150, 8 + i)[0], 150) for i in range(2)]
    mixed = [_mixed(s.genomes, (100, 190, 250, 300, 1000), 60, 20 + i) for i in range(2)]
    batches = [fixed[0], mixed[0], fixed[1]] if order == "fixed-mixed-fixed" else [mixed[0], fixed[0], mixed[1]]
    m, o = _run(s, batches)
    _check(o, m, order)
    m.close()


@pytest.mark.parametrize("positions", [128, 129])
def test_boundary_lengths(stores, positions):
    """128 k-mer positions: the last length with nothing launched behind the match kernel; 129: every read is a long one"""
    s = stores("rec31")
    length = s.k + positions - 1
    m, o = _run(s, [(_reads(s.genomes, N, length, 30 + positions)[0], length)] * 2)
    _check(o, m, "%d positions" % positions)
    m.close()


def test_striped_store_unchanged(stores):
    """two stripes on one device: the kernels write the bitmap themselves, the reset clears it, the old count kernels read it"""
    s = stores("rec31")
    stripes = ga.DeviceKMerStore.striped(s.k, s.kmers, s.vidx, s.n_values, s.parent, devices=(0, 0))
    a, b = (_reads(s.genomes, N, 150, 40, rows=range(0, 10))[0], 150), _reads(s.genomes, 500, 200, 41, rows=range(10, 20))
    m = ga.FastqKMerMatcher(stripes[0])
    o = _Oracle(s)
    o.submit(a, 0)
    _submit(m, a, 0)
    _check(o, m, "striped, batch A")
    m.reset()
    o = _Oracle(s)
    o.submit(b, 0)
    _submit(m, b, 0)
    _check(o, m, "striped, batch B after reset")
    m.close()
    for st in stripes:
        st.close()
