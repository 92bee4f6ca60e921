"""The index goal on the device (gs_index.hip; include/gsgpu.h gs_bloom_build_db, gs_bloom_get_info, gs_bloom_save / _load):
BloomIndexGoal over every kind of store, requested set and filter kind.  The expected keys are the input pairs filtered by the
export's contract (fastqgen.stored_pairs) and by requested[value]; the expected filter is the oracle's, sized for their count and
filled with put_many.  Every comparison is exact: geometry, hash factors, every word, the count."""
import os

import numpy as np
import pytest

import bloomref
import genestrip_amd as ga
from fastqgen import revcomp_np, stored_pairs
from genestrip_amd import synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

XOR, MURMUR, BLOCKED = ga.BLOOM_XOR, ga.BLOOM_MURMUR, ga.BLOOM_BLOCKED
UNSUPPORTED = -4
# (kind, fpp): XOR at the goal's default (27 hashes at realistic counts), one hash, 64 hashes; Murmur; blocked (fpp ignored)
KINDS = {"xor-1e-8": (XOR, 1e-8), "xor-0.5": (XOR, 0.5), "xor-64-hashes": (XOR, bloomref.fpp_for_hashes(64)),
         "murmur-1e-4": (MURMUR, 1e-4), "blocked": (BLOCKED, 0.01)}


class Case:
    """a store, the arrays it was built from, and the pairs it must hold"""

    def __init__(self, k, kmers, vidx, n_values, parent, marks, store=None):
        self.k, self.n_values, self.parent, self.marks = k, n_values, np.asarray(parent, dtype=np.int32), marks
        self.kmers, self.vidx = kmers, vidx
        self.store = store or ga.DeviceKMerStore(k, kmers, vidx, n_values, parent)
        self.keys, self.vals = stored_pairs(kmers, vidx, parent, k)
        assert self.store.info.n_stored == len(self.keys)

    def selected(self, requested):
        return self.keys[np.asarray(requested)[self.vals] != 0]


def _seeded(db, seed=3):
    """SynthDB arrays plus pairs the store must drop -- non-canonical keys (revcomp of stored ones), a value without a tree node --
    two more leaves under the root (`single` holds exactly one stored k-mer, `few` 300) and 150 k-mers on a genus node"""
    rng = np.random.default_rng(seed)
    k = db.k
    kmers, vidx = db.kmers.copy(), db.value_idx.copy()
    pick = rng.choice(len(kmers), 300, replace=False)
    rc = revcomp_np(kmers[pick], k)
    rc = rc[rc != kmers[pick]]  # (palindromes are their own reverse complement)
    single, few, no_node = db.n_values, db.n_values + 1, db.n_values + 2
    parent = np.concatenate([db.parent_vi, [0, 0, -2]]).astype(np.int32)
    moved = rng.choice(len(kmers), 651, replace=False)
    vidx[moved[:200]] = no_node
    vidx[moved[200:500]] = few
    vidx[moved[500]] = single
    internal = int(db.parent_vi[db.species_vi[0]])  # a genus: it holds k-mers of its own whatever the genomes share
    vidx[moved[501:]] = internal
    kmers = np.concatenate([kmers, rc])
    vidx = np.concatenate([vidx, rng.integers(1, db.n_values, len(rc)).astype(np.int32)])
    o = np.argsort(kmers)
    marks = dict(species=db.species_vi, internal=internal, single=single, few=few, no_node=no_node)
    return kmers[o], vidx[o], no_node + 1, parent, marks


def _synth_case(k):
    db = synth.SynthDB(k=k, genera=3, species_per_genus=3, genome_len=20000, seed=11)
    c = Case(k, *_seeded(db))
    c.genomes = db.genomes
    assert (c.store.info.n_in_records > 0) == (k >= 19)  # k < 19: table-only
    return c


def _ctx_case():
    old = os.environ.get("GS_GATE_CTX_MIN_DISTINCT")
    os.environ["GS_GATE_CTX_MIN_DISTINCT"] = "1"  # k = 22 with the context-keyed gate
    try:
        return _synth_case(22)
    finally:
        if old is None:
            del os.environ["GS_GATE_CTX_MIN_DISTINCT"]
        else:
            os.environ["GS_GATE_CTX_MIN_DISTINCT"] = old


def _many_values_case():
    """more than 2^21 values: the requested bitmap does not fit the LDS, and the store is table-only at k = 31"""
    k, nv = 31, (1 << 21) + 100
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 62, 408_000, dtype=np.int64) & ((1 << (2 * k)) - 1)
    kmers = np.unique(np.maximum(x, revcomp_np(x, k)))[:400_000]
    vidx = np.random.default_rng(6).integers(0, nv, len(kmers)).astype(np.int32)
    parent = np.zeros(nv, dtype=np.int32)
    parent[0] = -1
    parent[1::97] = -2  # values without a node
    c = Case(k, kmers, vidx, nv, parent, dict(species=np.flatnonzero(np.random.default_rng(7).integers(0, 2, nv))))
    assert c.store.info.n_in_records == 0
    return c


def _skewed_case():
    """a high overflow share: k-mers on both sides of the seam between record lines and table buckets"""
    env = {"GS_REC_LOAD": "0.5", "GS_REC_ROUNDS": "2"}
    old = {n: os.environ.get(n) for n in env}
    os.environ.update(env)
    try:
        db = synth.SkewedDB(genera=3, species_per_genus=3, genome_len=150_000, strains=2, dominant_len=1000, n_values=700, seed=12)
        seq, off, nvi = db.regions()
        gb = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
        gb.add(seq, off, nvi, update=False)
        gb.add(seq, off, nvi, update=True)
        kmers, vidx = gb.finish()
        gb.close()
        c = Case(31, kmers, vidx, db.n_values, db.parent_vi, dict(species=db.species_vi))
    finally:
        for n, v in old.items():
            if v is None:
                del os.environ[n]
            else:
                os.environ[n] = v
    i = c.store.info
    assert i.n_in_records > 0 and i.n_stored - i.n_in_records > 0.005 * i.n_stored
    return c


MAKERS = {"k31": lambda: _synth_case(31), "k22-ctx": _ctx_case, "k19": lambda: _synth_case(19), "k17": lambda: _synth_case(17),
          "k15": lambda: _synth_case(15), "many-values": _many_values_case, "skewed": _skewed_case}


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = MAKERS[name]()
        return made[name]
    yield get
    for c in made.values():
        c.store.close()


def _mask(c, values):
    m = np.zeros(c.n_values, dtype=np.uint8)
    m[np.asarray(values, dtype=np.int64)] = 1
    return m


def _requested(c, which):
    if which == "none":
        return _mask(c, [])
    if which == "all":
        return np.ones(c.n_values, dtype=np.uint8)
    if which == "species":
        return _mask(c, c.marks["species"])
    return _mask(c, [c.marks[which]])  # internal (the node, not its subtree), no_node, single, few


FIRST_FACTOR = synth.java_random_longs(42, 1)


def _oracle(kind, keys, fpp, expected=None):
    """the reference's filter: ensureExpectedSize(count) of its kind, then putLong of every key"""
    n = len(keys) if expected is None else expected
    if kind == BLOCKED:
        o = orc.Bloom(kind, max(n, 1), 0.01)
    elif n == 0:
        o = orc.Bloom.raw(kind, 1, 1, FIRST_FACTOR)  # (the oracle's constructor divides by the count)
    else:
        o = orc.Bloom(kind, n, fpp)
    o.put_many(keys)
    return o


def _check(bloom, o, kind, count, what=""):
    bits, factors, words = bloom.get()
    info = bloom.info()
    nh = 1 if kind == BLOCKED else o.hashes  # (a blocked filter has one seed; the oracle reports 0 hashes for it)
    assert (bits, info.bits, info.n_hashes, info.kind) == (o.bits, o.bits, nh, kind), what
    assert np.array_equal(factors, o.hash_factors[:nh]), what
    want = o.words
    assert info.n_words == len(words) == len(want), what
    assert np.array_equal(words, want), (what, int((words != want).sum()))
    assert info.n_inserted == count, what
    return words


def _build_and_check(c, requested, kind, fpp, what):
    keys = c.selected(requested)
    o = _oracle(kind, keys, fpp)
    bloom = ga.DeviceBloomFilter.from_store(c.store, requested, kind=kind, fpp=fpp)
    try:
        words = _check(bloom, o, kind, len(keys), what)
        info = bloom.info()
        assert info.k == c.k and info.expected_insertions == len(keys)
        assert info.fpp == (0.0 if kind == BLOCKED else fpp)
    finally:
        bloom.close()
        o.close()
    return keys, words


@pytest.mark.parametrize("kind_name", sorted(KINDS))
@pytest.mark.parametrize("store_name", sorted(MAKERS))
def test_every_store_and_kind(cases, store_name, kind_name):
    c = cases(store_name)
    kind, fpp = KINDS[kind_name]
    requested = _requested(c, "species")
    keys, words = _build_and_check(c, requested, kind, fpp, (store_name, kind_name))
    assert 0 < len(keys) < len(c.keys) and words.any()
    if kind_name == "xor-64-hashes":
        assert bloomref.geometry(len(keys), fpp)[1] == 64
    if kind_name == "xor-1e-8":
        assert bloomref.geometry(len(keys), fpp)[1] == 27
    if kind_name == "xor-0.5":
        assert bloomref.geometry(len(keys), fpp)[1] == 1


@pytest.mark.parametrize("kind_name", ["xor-1e-8", "murmur-1e-4", "blocked"])
@pytest.mark.parametrize("which", ["none", "all", "species", "internal", "no_node", "single", "few"])
@pytest.mark.parametrize("store_name", ["k31", "k17"])
def test_requested_sets(cases, store_name, which, kind_name):
    c = cases(store_name)
    kind, fpp = KINDS[kind_name]
    keys, words = _build_and_check(c, _requested(c, which), kind, fpp, (store_name, which, kind_name))
    if which in ("none", "no_node"):
        assert len(keys) == 0 and not words.any()
        if kind != BLOCKED:
            assert len(words) == 1  # bits = 1, one hash
    elif which == "all":
        assert len(keys) == len(c.keys)
    elif which == "internal":
        sub = c.selected(_mask(c, np.flatnonzero(c.parent == c.marks["internal"])))
        assert len(keys) >= 150 and len(sub) > 0  # the genus holds k-mers of its own, and so do its species: they are not selected
    elif which == "single":
        assert len(keys) == 1
        if kind_name == "xor-1e-8":
            assert bloomref.geometry(1, 1e-8) == (38, 26)
            bloom = ga.DeviceBloomFilter.from_store(c.store, _requested(c, which))
            assert (bloom.info().bits, bloom.info().n_hashes) == (38, 26)
            bloom.close()
    elif which == "few":
        assert len(keys) == 300
    else:
        assert 300 < len(keys) < len(c.keys)


def test_sixty_five_hashes_are_unsupported(cases):
    c = cases("k31")
    requested = _requested(c, "species")
    fpp = bloomref.fpp_for_hashes(65)
    assert bloomref.geometry(len(c.selected(requested)), fpp)[1] == 65
    with pytest.raises(ga.GsError) as e:
        ga.DeviceBloomFilter.from_store(c.store, requested, kind=XOR, fpp=fpp)
    assert e.value.code == UNSUPPORTED


def test_expected_insertions_above_2_32_bits(cases):
    """a few hundred keys in a filter whose bit index does not fit 32 bits: the set words against bloomref's indices"""
    c = cases("k31")
    requested = _requested(c, "few")
    keys = c.selected(requested)
    expected = 2_977_100_000
    bits, nh = bloomref.geometry(expected, 0.5)
    assert (1 << 32) < bits < (1 << 32) + (1 << 20) and nh == 1
    bloom = ga.DeviceBloomFilter.from_store(c.store, requested, kind=XOR, fpp=0.5, expected_insertions=expected)
    got_bits, factors, words = bloom.get()
    info = bloom.info()
    bloom.close()
    assert got_bits == bits and np.array_equal(factors, FIRST_FACTOR)
    assert (info.n_inserted, info.expected_insertions) == (len(keys), expected) and len(keys) == 300
    idx = bloomref.hash_index(XOR, factors, bits, keys).reshape(-1)
    assert idx.max() >= (1 << 31)  # (some of the 300 indices need the upper half of the range, a few all 33 bits)
    want = {}
    for i in idx.tolist():
        want[i >> 6] = want.get(i >> 6, 0) | (1 << (i & 63))
    at = np.flatnonzero(words)
    assert at.tolist() == sorted(want)
    assert words[at].tolist() == [want[w] for w in sorted(want)]


@pytest.mark.parametrize("kind_name", ["xor-1e-8", "blocked"])
def test_expected_insertions_equal_to_the_count(cases, kind_name):
    c = cases("k19")
    kind, fpp = KINDS[kind_name]
    requested = _requested(c, "species")
    a = ga.DeviceBloomFilter.from_store(c.store, requested, kind=kind, fpp=fpp)
    b = ga.DeviceBloomFilter.from_store(c.store, requested, kind=kind, fpp=fpp, expected_insertions=a.info().n_inserted)
    ga_, gb_ = a.get(), b.get()
    a.close()
    b.close()
    assert ga_[0] == gb_[0] and np.array_equal(ga_[1], gb_[1]) and np.array_equal(ga_[2], gb_[2])


def test_expected_insertions_other_than_the_count(cases):
    """the filter of a host that sized it elsewhere: the oracle's filter for that size, filled with the same keys"""
    c = cases("k31")
    requested = _requested(c, "species")
    keys = c.selected(requested)
    for kind, fpp in ((XOR, 1e-3), (BLOCKED, 0.01)):
        o = _oracle(kind, keys, fpp, expected=3 * len(keys) + 7)
        bloom = ga.DeviceBloomFilter.from_store(c.store, requested, kind=kind, fpp=fpp, expected_insertions=3 * len(keys) + 7)
        _check(bloom, o, kind, len(keys))
        assert bloom.info().expected_insertions == 3 * len(keys) + 7
        bloom.close()
        o.close()


@pytest.mark.parametrize("kind_name", sorted(KINDS))
def test_two_builds_give_equal_words(cases, kind_name):
    c = cases("skewed")
    kind, fpp = KINDS[kind_name]
    out = []
    for _ in range(2):
        bloom = ga.DeviceBloomFilter.from_store(c.store, _requested(c, "all"), kind=kind, fpp=fpp)
        out.append(bloom.get())
        bloom.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][2], out[1][2])


def test_beside_a_live_unique_counting_run(cases):
    """seen bits are set in records and table while the index is built: the index is that of the idle store, and the run's
    table is that of the same run without the build in between"""
    c = cases("k31")
    requested = _requested(c, "species")
    idle = ga.DeviceBloomFilter.from_store(c.store, requested)
    want = idle.get()
    idle.close()
    seq, off = synth.reads_host(c.genomes, 6000, read_len=150, seed=41)
    seq2, off2 = synth.reads_host(c.genomes, 6000, read_len=150, seed=42)
    m = ga.FastqKMerMatcher(c.store)
    m.match_reads(seq, off)
    for kind_name in ("xor-1e-8", "blocked"):
        kind, fpp = KINDS[kind_name]
        _build_and_check(c, requested, kind, fpp, "during the run")
    live = ga.DeviceBloomFilter.from_store(c.store, requested)
    during = live.get()
    live.close()
    m.match_reads(seq2, off2, first_read_no=6000)
    t1, _ = m.finish()
    m.close()
    assert during[0] == want[0] and np.array_equal(during[1], want[1]) and np.array_equal(during[2], want[2])
    m2 = ga.FastqKMerMatcher(c.store)
    m2.match_reads(seq, off)
    m2.match_reads(seq2, off2, first_read_no=6000)
    t2, _ = m2.finish()
    m2.close()
    assert t1[:, 3].sum() > 0 and np.array_equal(t1, t2)  # the unique column among them


@pytest.mark.parametrize("n_parts", [2, 3])
def test_a_partition_store_gives_the_filter_of_its_part(cases, n_parts):
    c = cases("k31")
    requested = _requested(c, "species")
    total = len(c.selected(requested))
    whole = ga.DeviceBloomFilter.from_store(c.store, requested, fpp=1e-4)
    union = np.zeros_like(whole.get()[2])
    seen = 0
    for p in range(n_parts):
        part = ga.DeviceKMerStore(c.k, c.kmers, c.vidx, c.n_values, c.parent, n_parts=n_parts, part=p)
        pk, pv = part.export()
        keys = pk[requested[pv] != 0]
        assert 0 < len(keys) < total
        for kind, fpp in ((XOR, 1e-4), (BLOCKED, 0.01)):
            o = _oracle(kind, keys, fpp)
            bloom = ga.DeviceBloomFilter.from_store(part, requested, kind=kind, fpp=fpp)
            _check(bloom, o, kind, len(keys), (p, kind))
            bloom.close()
            o.close()
        sized = ga.DeviceBloomFilter.from_store(part, requested, fpp=1e-4, expected_insertions=total)
        union |= sized.get()[2]
        seen += sized.info().n_inserted
        sized.close()
        part.close()
    assert seen == total and np.array_equal(union, whole.get()[2])  # the parts' filters, sized alike, OR to the whole store's
    whole.close()


def test_a_stripe_is_unsupported(cases):
    c = cases("k31")
    stripes = ga.DeviceKMerStore.striped(c.k, c.kmers, c.vidx, c.n_values, c.parent, devices=(0, 0))
    try:
        for s in stripes:
            with pytest.raises(ga.GsError) as e:
                ga.DeviceBloomFilter.from_store(s, _requested(c, "species"))
            assert e.value.code == UNSUPPORTED
    finally:
        for s in stripes:
            s.close()


@pytest.mark.parametrize("kind_name", ["xor-1e-8", "murmur-1e-4", "blocked"])
def test_save_load_round_trip(cases, tmp_path, kind_name):
    c = cases("k19")
    kind, fpp = KINDS[kind_name]
    requested = _requested(c, "species")
    bloom = ga.DeviceBloomFilter.from_store(c.store, requested, kind=kind, fpp=fpp)
    path = tmp_path / "species.gsindex"
    bloom.save(path)
    a, ia = bloom.get(), bloom.info()
    bloom.close()
    loaded = ga.DeviceBloomFilter.load(path)
    b, ib = loaded.get(), loaded.info()
    loaded.close()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[2].any()
    for f, _ in ga.BloomInfo._fields_:
        assert getattr(ia, f) == getattr(ib, f), f
    count = len(c.selected(requested))
    assert (ib.k, ib.n_inserted, ib.expected_insertions, ib.fpp) == (19, count, count, 0.0 if kind == BLOCKED else fpp)
    assert os.path.getsize(path) == 72 + 8 * (ib.n_hashes + ib.n_words)


def test_handles_of_the_older_calls_report_what_they_know(cases):
    c = cases("k17")
    keys = c.selected(_requested(c, "few"))
    built = ga.DeviceBloomFilter.build(keys, expected_insertions=1000, fpp=1e-3)
    i = built.info()
    assert (i.kind, i.k, i.expected_insertions, i.n_inserted, i.fpp) == (XOR, 0, 1000, 300, 1e-3)
    assert (i.bits, i.n_hashes) == bloomref.geometry(1000, 1e-3) and i.n_words == (i.bits + 63) // 64
    bits, factors, words = built.get()
    built.close()
    for kind, w in ((XOR, words), (BLOCKED, np.zeros(100 + 17, np.uint64))):
        made = ga.DeviceBloomFilter(kind, bits if kind == XOR else 100, factors, w)
        i = made.info()
        assert (i.kind, i.k, i.expected_insertions, i.n_inserted, i.fpp, i.n_words) == (kind, 0, -1, -1, 0.0, len(w))
        assert np.array_equal(made.get()[2], w)  # get() sizes its words from the handle: a blocked filter has buckets + 17
        made.close()


def _background(n, read_len, seed):
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n * read_len)]
    return seq, np.arange(n + 1, dtype=np.uint64) * np.uint64(read_len)


@pytest.mark.parametrize("kind_name", ["xor-1e-8", "murmur-1e-4", "blocked"])
@pytest.mark.parametrize("store_name,read_len", [("k31", 150), ("k15", 60)])
def test_the_goal_end_to_end(cases, tmp_path, store_name, read_len, kind_name):
    """index from the store -> file -> a fresh handle -> filter over reads that hit and reads that do not"""
    c = cases(store_name)
    kind, fpp = KINDS[kind_name]
    requested = _requested(c, "species")
    bloom = ga.DeviceBloomFilter.from_store(c.store, requested, kind=kind, fpp=fpp)
    path = tmp_path / "index.gsindex"
    bloom.save(path)
    bloom.close()
    loaded = ga.DeviceBloomFilter.load(path)
    hit, hoff = synth.reads_host(c.genomes, 1000, read_len=read_len, seed=77)
    bg, boff = _background(1000, read_len, 78)
    seq = np.concatenate([hit, bg])
    off = np.concatenate([hoff, hoff[-1] + boff[1:]]).astype(np.uint64)
    o = _oracle(kind, c.selected(requested), fpp)
    for min_pos, ratio in ((1, 0.2), (0, 0.2), (0, 0.9)):
        got = ga.FastqBloomFilter(c.k, loaded, min_pos_count=min_pos, positive_ratio=ratio).accept_reads(seq, off)
        want = o.filter_batch(c.k, min_pos, ratio, seq, off)
        assert np.array_equal(got, want), (min_pos, ratio, int((got != want).sum()))
        if (min_pos, ratio) == (0, 0.2):
            assert want[:1000].sum() > want[1000:].sum() and not want.all()  # reads of the indexed genomes pass, random ones do not
    loaded.close()
    o.close()
