"""Crowded slot tables: every reader of the 8-slot buckets (fused probe, gs_probe_keys_kernel, the slot decoders of export and index
build, the seen sweeps) and both builders (host loop, device passes) on tables with about five keys per bucket, where full home
buckets and chains of two and three full buckets are common, with and without the L2 word gate.

Every host-built layout is built under GS_BUCKET_LOAD = 4.85 with 39 720 k-mers, just under 4.85 * 2^13 (4.85 keys per bucket).  At 5.0
none of 200 random subsets found a place for every key within three buckets (the table doubles and the test goes empty); at 4.85
about one subset in 150 does, and those are the seeds below.  tests/planarkey.py (place) predicts bucket count, largest displacement
and every slot from the keys in input order; sizes and seeds were chosen with it on the CPU.  The preconditions, asserted again by
every run and printed with -s (displaced = share of the stored keys outside their home bucket):

  layout                                             seed       k-mers   buckets   max disp   displaced
  k16             k = 16, table only                 5          39 720   8 192     3          2.1 %
  k31-no-records  k = 31, GS_RECORDS=0               23         39 720   8 192     3          2.1 %
  k31-word-gate   k = 31, GS_MGATE=0 (same arrays)   23         39 720   8 192     3          2.1 %
  part rank 0     k = 31, 2-part partition store     117        39 720   8 192     3          2.5 %
  part rank 1                                        323        39 720   8 192     3          2.3 %
  strains         k = 31, records + overflow table   2          73 167   4 096     3          (18 458 table keys: 4.51 per bucket)

Reads: the genomes tiled so that every stored k-mer is covered (the oracle's unique-k-mer column adds up to n_stored), every tile a
second time with one substituted base in twenty (absent k-mers that pass the minimizer gate and walk full chains), every other read
reverse-complemented, random reads, reads with N and lower case, reads shorter than k, an empty read.  k = 31 layouts also hold the
remainder-zero keys (h < n_buckets, made with planarkey.unmix), every other one stored."""
import numpy as np
import pytest
import torch

import genestrip_amd as ga
import matchcheck
import planarkey as pk
import splitpipe
from fastqgen import stored_pairs
from genestrip_amd import synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

LOAD = 4.85
BITS = 13
NB = 1 << BITS
L = 150
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTNacgtn", b"TGCANtgcan"):
    COMP[_a] = _b
# layout -> (k, genome length of the nine synthetic genomes, subset seed and stored k-mers per owner rank); chosen with planarkey.place
DATASETS = {"k16": (16, 5600, (5,), (39720,)), "k31": (31, 11000, (23,), (39720,)), "part": (31, 11000, (117, 323), (39720, 39720))}


def rem_zero(k=31, nb=NB):
    """(h, canonical k-mer int64, bases uint8[n, k]) of the keys h < nb whose unmixed planes are the representative orientation"""
    h = np.arange(nb, dtype=np.uint64)
    hi, lo = pk.unmix_np(h)
    rhi, rlo = pk.rep_np(hi, lo, k)
    own = (rhi == hi) & (rlo == lo)
    h, hi, lo = h[own], hi[own], lo[own]
    codes = np.stack([(((hi >> np.uint64(i)) & np.uint64(1)) << np.uint64(1)) | ((lo >> np.uint64(i)) & np.uint64(1)) for i in range(k)], axis=1)
    return h.astype(np.int64), pk.kmers_of_planes_np(hi, lo, k), np.frombuffer(b"CGAT", dtype=np.uint8)[codes.astype(np.int64)]


class Data:
    """arrays of one store (k-mers ascending), the reads, the oracle's result over them"""

    def __init__(self, name):
        self.name = name
        self.k, glen, self.seed, counts = DATASETS[name]
        k = self.k
        db = synth.SynthDB(k=k, genera=3, species_per_genus=3, genome_len=glen, seed=11)
        self.n_values, self.parent_vi, self.genomes = db.n_values, db.parent_vi, db.genomes
        kmers, vidx = db.kmers, db.value_idx
        self.rz = None
        packed = []
        counts = list(counts)
        if k == 31:
            h, zk, zb = rem_zero()
            stored = np.arange(len(h)) % 2 == 0
            zv = (1 + np.arange(len(h)) % (self.n_values - 1)).astype(np.int32)
            assert not np.isin(zk, kmers).any() and len(np.unique(zk)) == len(zk)
            self.rz = dict(h=h, kmers=zk, bases=zb, stored=stored, values=zv)
            counts[0] -= int(stored.sum())  # (owner 0 of any world: h < 2^40)
            # four of them per read, every other k-mer from the other strand (the k-mers across the joints are random ones)
            zr = zb.copy()
            zr[1::2] = COMP[zb[1::2, ::-1]]
            packed = [zr[i:i + 4].reshape(-1) for i in range(0, len(zr), 4)]
        # a random subset of the genomes' k-mers: one draw, or one per owner rank for the two-rank partition store
        owner = (pk.keys_of_kmers_np(kmers, k) >> pk.OWNER_SHIFT) % len(counts)
        keep = []
        for p, (seed, n_p) in enumerate(zip(self.seed, counts)):
            mine = np.flatnonzero(owner == p)
            assert len(mine) >= n_p, (name, p, len(mine), n_p)
            keep.append(np.random.default_rng(seed).choice(mine, n_p, replace=False))
        keep = np.sort(np.concatenate(keep))
        kmers, vidx = kmers[keep], vidx[keep]
        rng = np.random.default_rng(99)
        if k == 31:
            kmers = np.concatenate([kmers, self.rz["kmers"][stored]])
            vidx = np.concatenate([vidx, self.rz["values"][stored]])
            o = np.argsort(kmers)
            kmers, vidx = kmers[o], vidx[o]
        self.kmers, self.vidx = np.ascontiguousarray(kmers), np.ascontiguousarray(vidx.astype(np.int32))
        self.keys = pk.keys_of_kmers_np(self.kmers, k)
        self.vbits, self.b0 = pk.value_bits(self.n_values)
        self._reads(rng, packed)
        self._placed = {}
        self._oracle = None

    def _reads(self, rng, packed):
        k, step = self.k, L - self.k + 1
        tiles, tails = [], []
        for g in self.genomes:
            for p in range(0, len(g) - k + 1, step):
                (tiles if p + L <= len(g) else tails).append(g[p:p + L])
        tiles = np.array(tiles)
        sub = tiles.copy()
        cols = np.arange(7, L, 20)
        sub[:, cols] = ACGT[(np.searchsorted(ACGT, sub[:, cols]) + rng.integers(1, 4, (len(sub), len(cols)))) % 4]
        both = np.concatenate([tiles, sub])
        both[1::2] = COMP[both[1::2, ::-1]]
        fixed = np.concatenate([both, ACGT[rng.integers(0, 4, (300, L))]])
        spoiled = tiles[:12].copy()
        for r in range(6):
            spoiled[r, (0, L // 2, L - 1)[r % 3]] = ord("N")
        for r in range(6, 12):
            a = (0, L // 2, L - 6)[r % 3]
            spoiled[r, a:a + 6] |= 0x20
        g = self.genomes[0]
        ragged = tails + list(spoiled) + packed + [g[:k - 1], g[:k], g[5:5 + k + 1], np.zeros(0, np.uint8), g[:3], g[40:40 + 2 * L + 7]]
        self.n_fixed = len(fixed)
        lens = np.concatenate([np.full(len(fixed), L), [len(r) for r in ragged]]).astype(np.uint64)
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.seq = np.ascontiguousarray(np.concatenate([fixed.reshape(-1)] + ragged).astype(np.uint8))

    def placed(self, part=None):
        """planarkey.place over the keys the host builder lays out: all of them, or rank `part`'s of two, in input order"""
        if part not in self._placed:
            mine = np.ones(len(self.keys), dtype=bool) if part is None else ((self.keys >> pk.OWNER_SHIFT) % 2) == part
            b, slots, md = pk.place(self.keys[mine], self.vidx[mine], self.b0, LOAD, self.vbits)
            self._placed[part] = dict(b=b, slots=slots, max_disp=md, n=int(mine.sum()), displaced=pk.displaced_share(slots, self.vbits))
        return self._placed[part]

    def oracle(self):
        if self._oracle is None:
            self.odb = orc.DB(self.k, self.kmers, self.vidx, self.n_values, self.parent_vi)
            self._oracle = matchcheck.oracle_batch(self.odb, self.seq, self.off)
            # the reads cover every stored k-mer
            assert int(self._oracle["table"][:, orc.C_UNIQUE_KMERS].sum()) == len(self.kmers)
        return self._oracle


STRAINS = dict(seed=2, base_len=5679, strains=20, rate=0.03)
STRAIN_BUCKETS = 1 << 12


class StrainData(Data):
    """near-identical strains of one random genome (substitutions at `rate`): around most minimizers the strains differ, a minimizer
    has two record buckets, so the windows of the third and later strains go to the overflow table, which the device passes build"""

    def __init__(self, seed, base_len, strains, rate):
        self.name, self.k, self.seed, self.rz = "strains", 31, (seed,), None
        tree = synth.SynthDB(k=31, genera=1, species_per_genus=strains, genome_len=64, seed=1, build=False)
        self.n_values, self.parent_vi = tree.n_values, tree.parent_vi
        rng = np.random.default_rng(seed)
        base = ACGT[rng.integers(0, 4, base_len)]
        self.genomes = np.empty((strains, base_len), dtype=np.uint8)
        ks, vs = [], []
        for s in range(strains):
            g = base.copy()
            pos = np.flatnonzero(rng.random(base_len) < rate)
            g[pos] = ACGT[(np.searchsorted(ACGT, g[pos]) + rng.integers(1, 4, len(pos))) % 4]
            self.genomes[s] = g
            u = np.unique(synth.canonical_kmers(g, 31))
            ks.append(u)
            vs.append(np.full(len(u), tree.species_vi[s], dtype=np.int32))
        allk, allv = np.concatenate(ks), np.concatenate(vs)
        o = np.argsort(allk, kind="stable")
        allk, allv = allk[o], allv[o]
        first = np.concatenate([[True], allk[1:] != allk[:-1]])
        starts = np.flatnonzero(first)
        vmin, vmax = np.minimum.reduceat(allv, starts), np.maximum.reduceat(allv, starts)
        # a k-mer of one strain carries that strain, a shared one the genus (value index 1)
        self.kmers, self.vidx = np.ascontiguousarray(allk[first]), np.where(vmin == vmax, vmin, 1).astype(np.int32)
        self.vbits, self.b0 = pk.value_bits(self.n_values)
        self._reads(rng, [])
        self._oracle = None


@pytest.fixture(scope="module")
def data():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Data(name)
        return made[name]
    return get


def _env(monkeypatch, gate, **more):
    monkeypatch.setenv("GS_BUCKET_LOAD", str(LOAD))
    if not gate:
        monkeypatch.setenv("GS_GATE_MAX_BYTES", "0")
    for name, v in more.items():
        monkeypatch.setenv(name, v)


def _check_crowded(d, info, gate, part=None):
    """the conditions that keep a run from going empty, from planarkey.place and from the store's own info"""
    p = d.placed(part)
    print(f"\n{d.name}{'' if part is None else ' rank %d' % part}: seed {d.seed}, {p['n']} k-mers, {1 << p['b']} buckets, "
          f"max displacement {p['max_disp']}, displaced {100 * p['displaced']:.1f} %, gate {info.gate_bytes} bytes")
    assert p["b"] == BITS and p["max_disp"] == pk.MAX_DISP and p["displaced"] >= 0.02
    assert 4.5 <= p["n"] / NB <= LOAD
    assert info.n_stored == p["n"] and info.n_in_records == 0 and info.rec_bytes == 0
    assert info.n_buckets == 1 << p["b"] and info.max_displacement == p["max_disp"] and info.value_bits == d.vbits
    assert (info.gate_bytes > 0) == gate


def _run_fused(store, d, split):
    """one run over d's reads: in one ragged batch, or (split) the reads of 150 bases as a fixed-length batch and the rest behind"""
    m = ga.FastqKMerMatcher(store)
    try:
        return _run_on(m, d, split)
    finally:
        m.close()


def _run_on(m, d, split):
    n = len(d.off) - 1
    if not split:
        cv, fl = m.match_reads(d.seq, d.off)
    else:
        nf = d.n_fixed
        cv = np.full(n, -1, dtype=np.int32)
        fl = np.zeros(n, dtype=np.uint8)
        m.submit_fixed(d.seq[:nf * L], L, nf, 0, class_vi=cv[:nf], flags=fl[:nf])
        m.submit(d.seq[nf * L:], np.ascontiguousarray(d.off[nf:] - d.off[nf]), nf, cv[nf:], fl[nf:])
    t, dt = m.finish()
    return dict(table=t, dtable=dt, class_vi=cv, flags=fl)


def _check_read_back(store, d):
    """the slot decoders: k-mer export and the index filter built from the device store"""
    want_k, want_v = stored_pairs(d.kmers, d.vidx, d.parent_vi, d.k)
    got_k, got_v = store.export()
    assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v)
    assert np.array_equal(store.value_counts(), np.bincount(want_v, minlength=d.n_values))
    fpp = 1e-6
    bloom = ga.DeviceBloomFilter.from_store(store, np.ones(d.n_values, dtype=np.uint8), kind=ga.BLOOM_XOR, fpp=fpp)
    o = orc.Bloom(ga.BLOOM_XOR, len(want_k), fpp)
    try:
        o.put_many(want_k)
        bits, factors, words = bloom.get()
        assert bits == o.bits and bloom.info().n_inserted == len(want_k)
        assert np.array_equal(factors, o.hash_factors[:o.hashes])
        assert np.array_equal(words, o.words), int((words != o.words).sum())
    finally:
        bloom.close()
        o.close()


def _check_fused_store(store, d, tmp_path, what):
    o = d.oracle()
    m = ga.FastqKMerMatcher(store)
    first = _run_on(m, d, split=False)
    matchcheck.check_match(o, first, what)
    m.reset()  # the seen bits of home and displaced slots are cleared: the unique column counts them again
    again = _run_on(m, d, split=True)
    m.close()
    matchcheck.check_match(o, again, what + ", after reset")
    _check_read_back(store, d)  # (the seen bits of the run are still set in the slots)
    path = tmp_path / "crowded.gss"
    store.save(path)
    loaded = ga.DeviceKMerStore.load(path)
    try:
        a, b = store.info, loaded.info
        assert (a.max_displacement, a.n_buckets, a.gate_bytes, a.mgate_bytes, a.n_stored) == \
               (b.max_displacement, b.n_buckets, b.gate_bytes, b.mgate_bytes, b.n_stored)
        matchcheck.check_match(o, _run_fused(loaded, d, split=False), what + ", loaded")
    finally:
        loaded.close()


FUSED = {"k16": ("k16", {}), "k31-no-records": ("k31", {"GS_RECORDS": "0"}), "k31-word-gate": ("k31", {"GS_MGATE": "0"})}


@pytest.mark.parametrize("gate", [True, False], ids=["gate", "no-gate"])
@pytest.mark.parametrize("layout", sorted(FUSED))
def test_host_built_fused_layouts(data, layout, gate, monkeypatch, tmp_path):
    name, env = FUSED[layout]
    d = data(name)
    _env(monkeypatch, gate, **env)
    store = ga.DeviceKMerStore(d.k, d.kmers, d.vidx, d.n_values, d.parent_vi)
    monkeypatch.undo()
    try:
        info = store.info
        _check_crowded(d, info, gate)
        assert (info.mgate_bytes > 0) == (layout == "k31-no-records")
        _check_fused_store(store, d, tmp_path, f"{layout}, gate {gate}")
    finally:
        store.close()


def _oracle_nodes(d, keys):
    """the oracle's lookup of the k-mers behind `keys` (planarkey: unmix -> planes -> the reference's canonical value)"""
    uniq, inv = np.unique(keys, return_inverse=True)
    km = pk.kmers_of_planes_np(*pk.unmix_np(uniq), d.k)
    return np.array([d.odb.get(int(x))[0] for x in km], dtype=np.int32)[inv]


@pytest.mark.parametrize("gate", [True, False], ids=["gate", "no-gate"])
def test_partition_layout(data, gate, monkeypatch):
    d = data("part")
    o = d.oracle()
    _env(monkeypatch, gate)
    stores = [ga.DeviceKMerStore(d.k, d.kmers, d.vidx, d.n_values, d.parent_vi, n_parts=2, part=p, partition=True) for p in range(2)]
    monkeypatch.undo()
    try:
        for p, s in enumerate(stores):
            _check_crowded(d, s.info, gate, part=p)
            assert s.info.mgate_bytes > 0
        res = splitpipe.run(stores, d.k, d.seq, d.off, device_routing=True)
        matchcheck.check_match_parts(o, res["parts"], f"two ranks, gate {gate}")
        n_hits = 0
        for p, (keys, nodes) in enumerate(res["probed"]):
            assert len(keys) > 30_000 and np.all((keys >> pk.OWNER_SHIFT) % 2 == p)
            want = _oracle_nodes(d, keys)
            bad = np.flatnonzero(nodes != want)
            assert bad.size == 0, (p, len(bad), keys[bad[:4]].tolist(), nodes[bad[:4]].tolist(), want[bad[:4]].tolist())
            n_hits += int((want >= 0).sum())
        assert n_hits >= len(d.kmers)
        # The minimizer gate of the encoding rank stops most absent k-mers before they are routed.  Straight to gs_probe_keys_kernel:
        # every stored key (a rank must miss the other rank's), every stored key with the lowest remainder bit flipped (same home
        # bucket, same chain, another remainder: absent unless stored by chance) and random keys
        rng = np.random.default_rng(5)
        probe = np.concatenate([d.keys, d.keys ^ (1 << BITS), rng.integers(0, 1 << pk.KEY_BITS, 50_000, dtype=np.int64)])
        want = _oracle_nodes(d, probe)
        assert (want[len(d.keys):] >= 0).sum() < 10
        for p, s in enumerate(stores):
            got = _probe(s, probe)
            mine = (probe >> pk.OWNER_SHIFT) % 2 == p
            bad = np.flatnonzero(got != np.where(mine, want, -1))
            assert bad.size == 0, (p, len(bad), probe[bad[:4]].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
        # the decoder of the export on both ranks' tables: their union is the input
        ex = [s.export() for s in stores]
        got_k, got_v = np.concatenate([e[0] for e in ex]), np.concatenate([e[1] for e in ex])
        order = np.argsort(got_k)
        assert np.array_equal(got_k[order], d.kmers) and np.array_equal(got_v[order], d.vidx)
    finally:
        for s in stores:
            s.close()


def _probe(store, keys):
    m = ga.FastqKMerMatcher(store)
    try:
        dk = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.int64)).cuda()
        nodes = torch.full((len(keys),), -9, dtype=torch.int32, device="cuda")
        m.probe_keys(dk, nodes, len(keys))
        m.sync()
        return nodes.cpu().numpy()
    finally:
        m.close()


@pytest.mark.parametrize("gate", [True, False], ids=["gate", "no-gate"])
@pytest.mark.parametrize("layout", ["k31-no-records", "partition"])
def test_remainder_zero_keys(data, layout, gate, monkeypatch):
    """keys with remainder 0 in their home bucket compare equal to an EMPTY slot once the value field is masked away
    (gs_match_bucket / gs_match_half: want == 0): a stored one must hit with its value, an absent one must miss whether its home
    bucket is empty, partly filled or full"""
    d = data("k31" if layout == "k31-no-records" else "part")
    z = d.rz
    _env(monkeypatch, gate, GS_RECORDS="0")
    if layout == "partition":
        store = ga.DeviceKMerStore(31, d.kmers, d.vidx, d.n_values, d.parent_vi, n_parts=2, part=0, partition=True)
    else:
        store = ga.DeviceKMerStore(31, d.kmers, d.vidx, d.n_values, d.parent_vi)
    monkeypatch.undo()
    try:
        info = store.info
        p = d.placed(0 if layout == "partition" else None)
        assert info.n_buckets == NB == 1 << p["b"] and info.n_in_records == 0 and (info.gate_bytes > 0) == gate
        h = z["h"]
        assert len(h) > NB // 3 and np.all(h >> BITS == 0) and np.all(h >> pk.OWNER_SHIFT == 0)  # remainder 0, owner 0
        assert np.array_equal(pk.keys_of_kmers_np(z["kmers"], 31), h)
        # what the absent ones find at home
        fill = (p["slots"].reshape(NB, pk.SLOTS) != 0).sum(axis=1)
        at_home = fill[h[~z["stored"]]]
        kinds = (int((at_home == 0).sum()), int(((at_home > 0) & (at_home < pk.SLOTS)).sum()), int((at_home == pk.SLOTS).sum()))
        print(f"\n{layout}: {int(z['stored'].sum())} stored and {len(at_home)} absent remainder-zero keys; the absent ones' home buckets: "
              f"{kinds[0]} empty, {kinds[1]} partly filled, {kinds[2]} full")
        assert min(kinds) > 0
        want = np.where(z["stored"], z["values"], -1).astype(np.int32)
        got = _probe(store, h)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (len(bad), h[bad[:6]].tolist(), got[bad[:6]].tolist(), want[bad[:6]].tolist())
        if layout == "k31-no-records":  # ... and through the fused kernels, one k-mer per read, every other one from the other strand
            reads = z["bases"].copy()
            reads[1::2] = COMP[reads[1::2, ::-1]]
            seq = np.ascontiguousarray(reads.reshape(-1))
            off = (np.arange(len(reads) + 1) * 31).astype(np.uint64)
            d.oracle()
            o = matchcheck.oracle_batch(d.odb, seq, off)
            assert int(o["table"][:, orc.C_UNIQUE_KMERS].sum()) == int(z["stored"].sum())
            m = ga.FastqKMerMatcher(store)
            cv, fl = m.match_reads(seq, off)
            t, dt = m.finish()
            m.close()
            matchcheck.check_match(o, dict(table=t, dtable=dt, class_vi=cv, flags=fl), "remainder-zero reads")
            kmers_col = ga.COLS.index("kmers")
            assert np.array_equal(t[:, kmers_col], np.bincount(z["values"][z["stored"]], minlength=d.n_values))
    finally:
        store.close()


def test_device_built_overflow_table(monkeypatch, tmp_path):
    """a fused k = 31 store with records whose overflow table is laid out by the device passes (gs_layout_build.hip).  They place
    in parallel, so planarkey.place predicts nothing here: bucket count, keys per bucket and the largest displacement are asserted
    from the store's info alone.  The device passes build no word gate (gate_bytes == 0 whatever GS_GATE_MAX_BYTES says), so
    there is one variant.  They place the keys of a bucket behind all keys whose home the next bucket is, which finds no place for
    some key sooner than the host's order: of eight seeds per size none kept 2^12 buckets at 4.53 keys per bucket, three did at
    4.3 .. 4.5, all with displacement 3.  Seed and genome length below: 18 458 table keys, 4.51 per bucket (the build is
    deterministic: two builds gave the same info)."""
    d = StrainData(**STRAINS)
    _env(monkeypatch, gate=True)
    store = ga.DeviceKMerStore(31, d.kmers, d.vidx, d.n_values, d.parent_vi)
    monkeypatch.undo()
    try:
        info = store.info
        n_table = info.n_stored - info.n_in_records
        print(f"\nstrains: seed {d.seed}, {info.n_stored} k-mers, {n_table} of them in {info.n_buckets} table buckets "
              f"({n_table / info.n_buckets:.2f} per bucket), max displacement {info.max_displacement}")
        assert info.n_stored == len(d.kmers) and info.n_in_records > 0 and info.rec_bytes > 0
        assert info.gate_bytes == 0 and info.mgate_bytes > 0
        assert info.n_buckets == STRAIN_BUCKETS and 4.5 <= n_table / info.n_buckets <= LOAD
        assert info.max_displacement == pk.MAX_DISP
        _check_fused_store(store, d, tmp_path, "device-built overflow table")
    finally:
        store.close()
