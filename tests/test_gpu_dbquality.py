"""gs_dbquality (the reference's dbqualcounts / dbquality goals, ft/.../finertree/goals/DBQualityCountsGoal.java handleStore :250-289):
per leaf tp / tp+fp / tp+fn of a store against its source genomes on the device -- the builder's k-mer kernel, two stable radix
sorts, a tiled merge join with the store in ascending order, per-leaf counts -- against the CPU reference of tests/qualitycheck.py
(unchanged oracle + numpy).  All counts are compared exactly, as integers.  Needs an MI355X: run with -m gpu."""
import os

import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
import qualitycheck as qc
from genestrip_amd import host, synth
from genestrip_amd.binding import kmer_ranges
from conftest import GOLDEN
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

# T/tax/TaxTreeLCATest.java:51 plus value 7 without a tree node
PARENT = np.array([-1, 0, 1, 1, 2, 4, 0, -2], dtype=np.int32)
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _revcomp(s):
    return s.translate(_COMP)[::-1]


def _device_counts(store, regions, lower=True, step=1, max_dust=-1, batches=1, handle=None):
    """regions: list of (bytes, leaf).  Batches alternate between host arrays and device tensors."""
    import torch
    q = handle or ga.DeviceDbQuality(store, lower_case_bases=lower, max_dust=max_dust, step_size=step)
    cuts = np.linspace(0, len(regions), batches + 1).astype(int)
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        part = regions[a:b]
        if not part:
            continue
        seq, off = qc.pack([s for s, _ in part])
        leaf = np.array([l for _, l in part], dtype=np.int32)
        if i % 2 == 1:
            q.add(torch.from_numpy(seq.copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), leaf)
        else:
            q.add(seq, off, leaf)
    counts, present = q.finish()
    if handle is None:
        q.close()
    return counts, present


def _oracle_store(k, fill, parent, lower, step, max_dust):
    ob = orc.DbBuild(k, len(parent), parent, lower, step, max_dust)
    seq, off = qc.pack([s for s, _ in fill])
    ob.fill(seq, off, np.array([n for _, n in fill], dtype=np.int32))
    ob.optimize()
    kmers, vals = ob.fetch()
    ob.close()
    return kmers, vals


def test_dengue_known_answer_on_the_device():
    raw = open(os.path.join(GOLDEN, "dengue1", "dengue1.fasta"), "rb").read()
    rd = orc.parse_fastq(raw, fasta=True, k=31)
    seq = bytes(rd["seq"])
    off = rd["seq_off"].astype(np.int64)
    regions = [(seq[off[i]:off[i + 1]], 1) for i in range(len(off) - 1)]
    kmers = np.unique(np.concatenate([orc.canonical_kmers(s.decode().upper(), 31) for s, _ in regions]))
    parent = np.array([-1, 0], np.int32)
    store = ga.DeviceKMerStore(31, kmers, np.ones(len(kmers), np.int32), 2, parent)
    counts, present = _device_counts(store, regions)
    assert counts.tolist() == [[0, 0, 0], [10705, 10705, 10705]] and present.tolist() == [0, 1]
    ref = qc.reference_counts(31, kmers, np.ones(len(kmers), np.int32), parent, regions)
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(present, ref["present"])
    store.close()


def _noisy_case(k, step, seed):
    """-> (regions, fill): explicit regions that show every case the sweep must cover, then random noisy ones"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    alphabet = np.frombuffer(b"ACGTacgtN\r", dtype=np.uint8)
    p = np.array([0.235, 0.235, 0.235, 0.235, 0.015, 0.015, 0.01, 0.01, 0.008, 0.002])
    core = rng.choice(acgt, 3000).tobytes()
    L = 800
    while (L + k) % step:
        L += 1  # (the windows of the reverse strand then fall on the same k-mers at this step)
    A = core[:L]
    sep = b"N" * (step - L % step)
    own5 = rng.choice(acgt, 1200).tobytes()
    left_out = rng.choice(acgt, 1500).tobytes()
    explicit = [
        (A + sep + A, 3),            # a k-mer twice in one region
        (A, 3),                      # ... and in two regions of one leaf
        (_revcomp(A), 3),            # ... and on both strands
        (A + b"N" + own5, 5),        # shared by two leaves; the store holds A under 3, which is off the path of 5
        (core[1000:2200], 1),        # a leaf that is an inner node of the tree
        (core[1000:2200] + b"N" + own5[:600], 4),
        (left_out + b"N" + core[1100:1400], 6),  # a genome the store was not filled with: most of its k-mers are not stored
        (A, -1),                     # no leaf node
        (A, 7),                      # a value without a tree node
        (b"", 2), (b"ACGT" * 3, 5),  # empty, shorter than k
    ]
    fill = [r for r in explicit[:6]]
    noisy = []
    for r in range(50):
        body = bytearray(rng.choice(alphabet, int(rng.integers(0, 2500)), p=p).tobytes())
        if r % 2 == 0 and len(body) > 900:
            a = int(rng.integers(0, 2000))
            body[100:900] = core[a:a + 800]
        if r % 5 == 0:  # low-complexity islands for the DUST filter
            unit = rng.choice(acgt, int(rng.integers(1, 4))).tobytes()
            body += b"N" + (unit * 80)[:int(rng.integers(40, 160))] + rng.choice(acgt, 50).tobytes()
        noisy.append((bytes(body), int(rng.integers(0, 7))))
    fill += noisy[::2]
    regions = explicit + noisy
    return regions, fill, dict(A=A, sep=sep, own5=own5, left_out=left_out)


DUST = {15: 16, 21: 24, 31: 36}  # about the mean score of a random k-mer: takes the upper tail and the islands out


@pytest.mark.parametrize("dust", [False, True])
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("k", [15, 21, 31])
def test_device_counts_equal_the_reference_on_noisy_regions(k, lower, step, dust):
    max_dust = DUST[k] if dust else -1
    regions, fill, parts = _noisy_case(k, step, 1000 * k + 10 * step + dust)
    # the store: the fill regions only (no update pass: the first region's node stays, so shared k-mers sit off other leaves'
    # paths), then some stored k-mers moved to the value without a tree node: the store drops those
    sk, sv = _oracle_store(k, fill, PARENT[:7], lower, step, max_dust)
    sv = sv.copy()
    moved = np.arange(len(sk)) % 11 == 5
    sv[moved] = 7
    ref = qc.reference_counts(k, sk, sv, PARENT, regions, lower, step, max_dust)
    rc, rp, distinct = ref["counts"], ref["present"], ref["distinct"]
    # ---- the reference side shows every case, before the device is looked at
    assert any(0 < rc[v, 0] < rc[v, 2] for v in range(8)), rc                      # a stored value off the leaf's path
    assert any(rp[v] and rc[v, 2] < distinct[v] for v in distinct), (rc, distinct)   # k-mers that are not stored
    A, sep = parts["A"], parts["sep"]
    one = qc.leaf_kmers(k, [A], lower, step, max_dust)
    assert len(one) > 100
    assert np.array_equal(qc.leaf_kmers(k, [A + sep + A], lower, step, max_dust), one)       # twice in one region
    assert np.array_equal(qc.leaf_kmers(k, [A, A], lower, step, max_dust), one)              # in two regions of one leaf
    assert np.array_equal(qc.leaf_kmers(k, [A, _revcomp(A)], lower, step, max_dust), one)    # on both strands
    five = qc.leaf_kmers(k, [s for s, l in regions if l == 5], lower, step, max_dust)
    three = qc.leaf_kmers(k, [s for s, l in regions if l == 3], lower, step, max_dust)
    assert len(np.intersect1d(three, five)) > 100 and rp[3] and rp[5]                       # shared by two leaves
    assert any(l < 0 for _, l in regions) and any(l == 7 for _, l in regions)
    assert not rp[7] and rc[7].tolist() == [0, 0, 0]
    assert moved.sum() > 0 and len(qc.stored_pairs(sk, sv, PARENT)[0]) == len(sk) - moved.sum()  # value without a node = not stored
    assert rp[1] and rp[4]                                                                   # inner nodes as leaves
    if max_dust >= 0:
        assert any(len(qc.leaf_kmers(k, [s for s, l in regions if l == v], lower, step, -1)) > distinct[v] for v in distinct)
    # ---- the device
    store = ga.DeviceKMerStore(k, sk, sv, 8, PARENT)
    counts, present = _device_counts(store, regions, lower, step, max_dust, batches=5)
    assert np.array_equal(present, rp), (present, rp)
    assert np.array_equal(counts, rc), (counts, rc)
    # one batch, host memory only: the same
    c1, p1 = _device_counts(store, regions, lower, step, max_dust, batches=1)
    assert np.array_equal(c1, rc) and np.array_equal(p1, rp)
    store.close()


@pytest.fixture(scope="module")
def skewed():
    """repeat-rich / shared-core genomes; one leaf owns >= 90 % of the regions; n_values above the kernel's LDS row limit"""
    db = synth.SkewedDB(genera=3, species_per_genus=4, genome_len=150_000, strains=2, dominant_len=2000, n_values=3000, seed=21)
    seq, off, node = db.regions()
    off = off.astype(np.int64)
    fill = [(seq[off[i]:off[i + 1]].tobytes(), int(node[i])) for i in range(len(node))]
    sk, sv = _oracle_store(31, fill, db.parent_vi, True, 1, -1)
    big = int(db.species_vi[0])
    regions = []
    for i, (s, v) in enumerate(fill):
        if i < 10:  # ten genomes in 1000-base regions under ONE leaf
            regions += [(s[a:a + 1000], big) for a in range(0, len(s), 1000)]
        else:
            regions.append((s, v))
    return db, sk, sv, regions, big


def test_skewed_collection_on_the_global_atomic_path(skewed):
    db, sk, sv, regions, big = skewed
    assert db.n_values > 2048 and sum(len(s) for s, _ in regions) >= 2_000_000
    assert sum(l == big for _, l in regions) >= 0.9 * len(regions)
    ref = qc.reference_counts(31, sk, sv, db.parent_vi, regions)
    assert ref["present"].sum() >= 4 and 0 < ref["counts"][big, 0] < ref["counts"][big, 2]
    store = ga.DeviceKMerStore(31, sk, sv, db.n_values, db.parent_vi)
    counts, present = _device_counts(store, regions, batches=3)
    assert np.array_equal(present, ref["present"])
    assert np.array_equal(counts, ref["counts"]), (counts[present > 0], ref["counts"][present > 0])
    store.close()


def test_kmer_ranges_add_up_to_one_run(skewed):
    db, sk, sv, regions, big = skewed
    regions = regions[::3]
    store = ga.DeviceKMerStore(31, sk, sv, db.n_values, db.parent_vi)
    whole, wp = _device_counts(store, regions)
    q = ga.DeviceDbQuality(store)
    total = np.zeros_like(whole)
    seen = np.zeros_like(wp)
    for lo, hi in kmer_ranges(31, 3):
        q.set_range(lo, hi)  # (after finish: the next pass on the same handle, the decoded store stays)
        c, p = _device_counts(store, regions, batches=2, handle=q)
        ref = qc.reference_counts(31, sk, sv, db.parent_vi, regions, lo=lo, hi=hi)
        assert np.array_equal(c, ref["counts"]) and np.array_equal(p, ref["present"])
        assert np.array_equal(c[p > 0, 1], whole[p > 0, 1])  # tp+fp does not depend on the range
        assert q.stats().n_found == c[:, 2].sum()
        total[:, [0, 2]] += c[:, [0, 2]]
        seen |= p
    q.close()
    assert np.array_equal(total[:, [0, 2]], whole[:, [0, 2]]) and np.array_equal(seen, wp)
    store.close()


def test_the_store_is_left_as_it_was():
    sdb = synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)
    g = sdb.genomes
    regions = [(g[i].tobytes(), int(sdb.species_vi[i])) for i in range(g.shape[0])]
    store = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    seq, off = synth.reads_host(g, 6000, read_len=150, seed=41)
    seq2, off2 = synth.reads_host(g, 6000, read_len=150, seed=42)

    def table():
        m = ga.FastqKMerMatcher(store)
        m.match_reads(seq, off)
        t, _ = m.finish()  # (the integer table; the double sums depend on the order of their atomics)
        m.close()
        return t
    vc0, t0 = store.value_counts(), table()
    ref = qc.reference_counts(31, sdb.kmers, sdb.value_idx, sdb.parent_vi, regions)
    counts, present = _device_counts(store, regions)
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(present, ref["present"])
    vc1, t1 = store.value_counts(), table()
    assert np.array_equal(vc0, vc1) and np.array_equal(t0, t1)
    # a quality run while a unique-counting run is alive on the store: seen bits are neither read as data nor written
    m = ga.FastqKMerMatcher(store)
    cv1, fl1 = m.match_reads(seq, off)
    counts2, present2 = _device_counts(store, regions, batches=2)
    cv2, fl2 = m.match_reads(seq2, off2, first_read_no=6000)
    t, d = m.finish()
    m.close()
    assert np.array_equal(counts2, ref["counts"]) and np.array_equal(present2, ref["present"])
    odb = orc.DB(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    o = matchcheck.oracle_batch(odb, np.concatenate([seq, seq2]), np.concatenate([off, off[-1] + off2[1:]]))
    assert t[:, 3].sum() > 0 and np.array_equal(t, o["table"])
    matchcheck.check_match(o, dict(table=t, dtable=d, class_vi=np.concatenate([cv1, cv2]), flags=np.concatenate([fl1, fl2])),
                           "quality run during a unique-counting run")
    odb.close()
    store.close()


def test_genomes_to_store_to_quality_csv(tmp_path):
    import torch
    db = synth.SynthDB(k=31, genera=3, species_per_genus=4, genome_len=40000, seed=5)
    g = db.genomes
    dseq = torch.from_numpy(np.ascontiguousarray(g).reshape(-1)).cuda()
    doff = torch.arange(g.shape[0] + 1, dtype=torch.int64, device="cuda") * g.shape[1]
    gb = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
    gb.add(dseq, doff, db.species_vi, update=False)
    gb.add(dseq, doff, db.species_vi, update=True)
    store = gb.to_store()
    gb.close()
    q = ga.DeviceDbQuality(store)
    q.add(dseq, doff, db.species_vi)
    counts, present = q.finish()
    st = q.stats()
    q.close()
    assert st.n_store == len(db.kmers) and st.n_found == counts[:, 2].sum() and st.n_pairs >= st.n_distinct >= st.n_found > 0
    depth = np.zeros(db.n_values, int)
    for v in range(db.n_values):
        a = db.parent_vi[v]
        while a >= 0:
            depth[v] += 1
            a = db.parent_vi[a]
    ranks = [("no rank", "genus", "species")[d] for d in depth]
    names = ["node %d" % v for v in range(db.n_values)]
    path = tmp_path / "quality.csv"
    host.write_quality_csv(path, db.parent_vi, db.taxids, counts, present, names=names, ranks=ranks)
    regions = [(g[i].tobytes(), int(db.species_vi[i])) for i in range(g.shape[0])]
    ref = qc.reference_counts(31, db.kmers, db.value_idx, db.parent_vi, regions)
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(present, ref["present"])
    want = qc.quality_csv(db.parent_vi, db.taxids, ref["counts"], ref["present"], names, ranks)
    assert path.read_bytes() == want
    lines = want.decode().split("\n")
    assert len(lines) == 1 + 3 + 12 + 1 and ";genus;" in lines[1]  # every species, and every genus by aggregation
    # a store against its own sources: every stored k-mer of a genome sits on its path (recall 1); the path may hold more
    assert all(0 < c[0] == c[2] <= c[1] for c in ref["counts"][db.species_vi])
    store.close()


def test_argument_errors():
    L = ga.lib()
    sdb = synth.SynthDB(k=31, genera=2, species_per_genus=2, genome_len=5000, seed=7)
    store = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    seq, off = qc.pack([b"ACGT" * 20, b"GATTACA" * 10])
    leaf = np.array([int(sdb.species_vi[0])] * 2, np.int32)

    def err(fn, code):
        with pytest.raises(ga.GsError) as e:
            fn()
        assert e.value.code == code and len(str(e.value).split(": ", 1)[1]) > 0, str(e.value)
    import ctypes as C
    h = C.c_void_p()
    assert L.gs_dbquality_begin(None, store.h, 1, -1, 1) == -1 and L.gs_last_error()
    assert L.gs_dbquality_begin(C.byref(h), None, 1, -1, 1) == -1 and L.gs_last_error() and not h.value
    assert L.gs_dbquality_add(None, None, None, None, 0, 0) == -1 and L.gs_dbquality_set_range(None, 0, 1) == -1
    assert L.gs_dbquality_finish(None, None, None) == -1 and L.gs_dbquality_get_stats(None, None) == -1
    assert L.gs_dbquality_destroy(None) == 0
    err(lambda: ga.DeviceDbQuality(store, step_size=0), -1)
    err(lambda: ga.DeviceDbQuality(store, max_dust=40000), -1)
    q = ga.DeviceDbQuality(store)
    err(lambda: q.add(seq, np.array([1, 80, 150], np.uint64), leaf), -1)   # offsets not from 0
    err(lambda: q.add(seq, np.array([0, 90, 80], np.uint64), leaf), -1)    # descending
    err(lambda: q.add(seq, off, np.array([0, sdb.n_values], np.int32)), -1)  # leaf_vi >= n_values
    err(lambda: q.set_range(5, 5), -1)
    assert L.gs_dbquality_finish(q.h, None, None) == -1
    q.add(seq, off, leaf)
    err(lambda: q.set_range(0, 5), -5)  # only before the first add of a pass
    counts, present = q.finish()         # the handle still works after the refused calls
    assert not present.any() and not counts.any()
    err(lambda: q.add(seq, off, leaf), -5)  # add after finish
    err(q.finish, -5)
    q.close()
    q.close()
    # a stripe of a striped store is refused
    stripe = ga.DeviceKMerStore.stripe(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, device=0, n_stripes=2, stripe=0)
    err(lambda: ga.DeviceDbQuality(stripe), -4)
    stripe.close()
    store.close()
