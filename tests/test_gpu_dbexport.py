"""The device store read back (gs_export.hip, include/gsgpu.h gs_db_value_counts / gs_dbexport_*, gshost.h gs_host_db2fastq):
KMerStore.visit, Database.getStats and the db2fastq goal over every kind of store, checked against the input arrays filtered by the
export's contract (tests/fastqgen.py) and against the reference's own db2fastq property (DB2FastqGoalTest)."""
import gzip

import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
from genestrip_amd import host, synth
from fastqgen import fastq_text, revcomp_np, stored_pairs, subtree
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _seeded(db, seed=3):
    """SynthDB arrays plus pairs the store must drop: non-canonical keys (revcomp of stored ones) and a value without a tree node"""
    rng = np.random.default_rng(seed)
    k = db.k
    kmers, vidx = db.kmers.copy(), db.value_idx.copy()
    pick = rng.choice(len(kmers), 300, replace=False)
    rc = revcomp_np(kmers[pick], k)
    rc = rc[rc != kmers[pick]]  # (palindromes are their own reverse complement)
    n_values = db.n_values + 1
    parent = np.concatenate([db.parent_vi, [-2]]).astype(np.int32)
    vidx[rng.choice(len(kmers), 200, replace=False)] = n_values - 1  # no tree node
    kmers = np.concatenate([kmers, rc])
    vidx = np.concatenate([vidx, rng.integers(1, db.n_values, len(rc)).astype(np.int32)])
    o = np.argsort(kmers)
    return kmers[o], vidx[o], n_values, parent


def _check_round_trip(store, k, kmers, vidx, parent):
    want_k, want_v = stored_pairs(kmers, vidx, parent, k)
    got_k, got_v = store.export()
    assert len(got_k) == store.info.n_stored == len(want_k)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_v, want_v)
    return got_k, got_v


@pytest.mark.parametrize("k", [31, 25, 22, 21, 19, 17, 15])
def test_round_trip(k, monkeypatch):
    """records (k >= 19; k = 22 with the context-keyed gate) and table-only stores (k < 19)"""
    if k == 22:
        monkeypatch.setenv("GS_GATE_CTX_MIN_DISTINCT", "1")
    db = synth.SynthDB(k=k, genera=3, species_per_genus=3, genome_len=20000, seed=11)
    kmers, vidx, nv, parent = _seeded(db)
    store = ga.DeviceKMerStore(k, kmers, vidx, nv, parent)
    i = store.info
    assert (i.n_in_records > 0) == (k >= 19)
    gk, gv = _check_round_trip(store, k, kmers, vidx, parent)
    assert np.array_equal(store.value_counts(), np.bincount(gv, minlength=nv))
    store.close()


def _random_canonical(n, k, seed):
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 1 << 62, int(n * 1.02), dtype=np.int64) & ((1 << (2 * k)) - 1))
    x = np.unique(np.maximum(x, revcomp_np(x, k)))
    return x[:n] if len(x) > n else x


def test_more_than_2_21_values_table_only():
    k, nv = 31, (1 << 21) + 100
    kmers = _random_canonical(400_000, k, 5)
    rng = np.random.default_rng(6)
    vidx = rng.integers(0, nv, len(kmers)).astype(np.int32)
    parent = np.zeros(nv, dtype=np.int32)
    parent[0] = -1
    parent[1::97] = -2  # values without a node (no children: every node's parent is the root)
    store = ga.DeviceKMerStore(k, kmers, vidx, nv, parent)
    assert store.info.n_in_records == 0
    _check_round_trip(store, k, kmers, vidx, parent)
    _, gv = store.export()
    assert np.array_equal(store.value_counts(), np.bincount(gv, minlength=nv))  # (global atomics: too many values for LDS)
    store.close()


def test_skewed_store_with_high_overflow_share(monkeypatch):
    monkeypatch.setenv("GS_REC_LOAD", "0.5")  # full record buckets, few cuckoo rounds: more windows go to the table
    monkeypatch.setenv("GS_REC_ROUNDS", "2")
    db = synth.SkewedDB(genera=3, species_per_genus=3, genome_len=150_000, strains=2, dominant_len=1000, n_values=700, seed=12)
    seq, off, nvi = db.regions()
    gb = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
    gb.add(seq, off, nvi, update=False)
    gb.add(seq, off, nvi, update=True)
    kmers, vidx = gb.finish()
    gb.close()
    store = ga.DeviceKMerStore(31, kmers, vidx, db.n_values, db.parent_vi)
    i = store.info
    assert i.n_stored - i.n_in_records > 0.005 * i.n_stored  # low-complexity islands, strains, homeless windows: k-mers in the table
    _check_round_trip(store, 31, kmers, vidx, db.parent_vi)
    store.close()


def test_forty_million_kmers():
    k = 31
    kmers = _random_canonical(40_500_000, k, 8)
    assert len(kmers) >= 40_000_000
    db = synth.SynthDB(k=k, genera=8, species_per_genus=8, genome_len=1000, seed=2, build=False)
    rng = np.random.default_rng(9)
    vidx = rng.integers(0, db.n_values, len(kmers)).astype(np.int32)
    store = ga.DeviceKMerStore(k, kmers, vidx, db.n_values, db.parent_vi)
    assert store.info.n_in_records > 0
    _check_round_trip(store, k, kmers, vidx, db.parent_vi)
    store.close()


def test_device_built_and_loaded_stores(tmp_path):
    import torch
    db = synth.SynthDB(k=31, genera=3, species_per_genus=4, genome_len=40000, seed=5, build=False)
    g = db.genomes
    dseq = torch.from_numpy(np.ascontiguousarray(g).reshape(-1)).cuda()
    doff = torch.arange(g.shape[0] + 1, dtype=torch.int64, device="cuda") * g.shape[1]
    gb = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
    gb.add(dseq, doff, db.species_vi, update=False)
    gb.add(dseq, doff, db.species_vi, update=True)
    kmers, vidx = gb.finish()
    store = gb.to_store()
    gb.close()
    gk, gv = store.export()
    assert np.array_equal(gk, kmers) and np.array_equal(gv, vidx)  # gs_dbbuild_to_db exports what gs_dbbuild_fetch returns
    path = tmp_path / "built.gss"
    store.save(path)
    store.close()
    loaded = ga.DeviceKMerStore.load(path)
    lk, lv = loaded.export()
    assert np.array_equal(lk, gk) and np.array_equal(lv, gv)
    loaded.close()


@pytest.fixture(scope="module")
def sdb():
    return synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)


@pytest.mark.parametrize("n_parts", [2, 3])
def test_partition_parts_union_is_the_whole(sdb, n_parts):
    whole = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    wk, wv = whole.export()
    ks, vs = [], []
    for p in range(n_parts):
        part = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, n_parts=n_parts, part=p)
        k_, v_ = part.export()
        assert len(k_) == part.info.n_stored and np.all(np.diff(k_) > 0)
        ks.append(k_)
        vs.append(v_)
        part.close()
    k_, v_ = np.concatenate(ks), np.concatenate(vs)
    o = np.argsort(k_)
    assert np.array_equal(k_[o], wk) and np.array_equal(v_[o], wv)
    whole.close()


def test_stripes_union_is_the_whole(sdb):
    whole = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    wk, wv = whole.export()
    stripes = ga.DeviceKMerStore.striped(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, devices=(0, 0))
    parts = [s.export() for s in stripes]
    assert all(len(p[0]) > 0 for p in parts)
    k_ = np.concatenate([p[0] for p in parts])
    v_ = np.concatenate([p[1] for p in parts])
    o = np.argsort(k_)
    assert np.array_equal(k_[o], wk) and np.array_equal(v_[o], wv)
    for s in stripes:
        s.close()
    whole.close()


def test_export_during_a_unique_counting_run(sdb):
    store = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    before = store.export()
    seq, off = synth.reads_host(sdb.genomes, 6000, read_len=150, seed=41)
    seq2, off2 = synth.reads_host(sdb.genomes, 6000, read_len=150, seed=42)
    m = ga.FastqKMerMatcher(store)
    cv1, fl1 = m.match_reads(seq, off)
    during = store.export()  # seen bits are set in records and table now
    counts = store.value_counts()
    cv2, fl2 = m.match_reads(seq2, off2, first_read_no=6000)
    t1, d1 = m.finish()
    m.close()
    assert np.array_equal(during[0], before[0]) and np.array_equal(during[1], before[1])
    assert np.array_equal(counts, np.bincount(before[1], minlength=sdb.n_values))
    m2 = ga.FastqKMerMatcher(store)
    m2.match_reads(seq, off)
    m2.match_reads(seq2, off2, first_read_no=6000)
    t2, d2 = m2.finish()
    m2.close()
    assert t1[:, 3].sum() > 0 and np.array_equal(t1, t2)  # the unique column among them
    odb = orc.DB(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    both = (np.concatenate([seq, seq2]), np.concatenate([off, off[-1] + off2[1:]]))
    o = matchcheck.oracle_batch(odb, *both)
    for t, d in ((t1, d1), (t2, d2)):
        matchcheck.check_match(o, dict(table=t, dtable=d, class_vi=np.concatenate([cv1, cv2]), flags=np.concatenate([fl1, fl2])),
                               "export during the run")
    store.close()


def test_selection_and_counts(sdb):
    store = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    ak, av = store.export()
    assert np.array_equal(store.value_counts(), np.bincount(av, minlength=sdb.n_values))
    leaf, internal, root = int(sdb.species_vi[1]), 1, 0
    for v in (leaf, internal, root):
        for desc in (False, True):
            keep = subtree(sdb.parent_vi, v)[av] if desc else av == v
            gk, gv = store.export(select=v, with_desc=desc)
            assert np.array_equal(gk, ak[keep]) and np.array_equal(gv, av[keep]), (v, desc)
            assert len(gk) > 0 or not desc  # (a genus or the root may hold no k-mer of its own)
    store.close()


@pytest.mark.parametrize("chunk", [None, "3000"])
def test_db2fastq_bytes(sdb, tmp_path, monkeypatch, chunk):
    """plain and .gz files byte for byte what KMerFastqGenerator + FastQWriter print; chunk: small text chunks (many seams)"""
    if chunk:
        monkeypatch.setenv("GS_EXPORT_CHUNK_BYTES", chunk)
    store = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    ak, av = store.export()
    leaf, genus = int(sdb.species_vi[2]), 2
    cases = {"total": (None, True, np.ones(len(av), dtype=bool)), "exact": (leaf, False, av == leaf),
             "plus": (genus, True, subtree(sdb.parent_vi, genus)[av])}
    for name, (sel, desc, keep) in cases.items():
        want = fastq_text(ak[keep], av[keep], sdb.taxids, 31, "proj")
        p = tmp_path / f"{name}.fastq"
        assert host.db2fastq(store, sdb.taxids, "proj", p, select=sel, with_desc=desc) == int(keep.sum())
        assert p.read_bytes() == want, name
        pz = tmp_path / f"{name}.fastq.gz"
        host.db2fastq(store, sdb.taxids, "proj", pz, select=sel, with_desc=desc)
        raw = pz.read_bytes()
        assert raw.endswith(BGZF_EOF) and gzip.decompress(raw) == want, name
    store.close()


def test_db2fastq_reads_match_back_to_their_taxid(sdb, tmp_path):
    """DB2FastqGoalTest: the FASTQ of one tax id, matched against the same store, hits that tax id with every k-mer once"""
    store = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    counts = store.value_counts()
    genera = np.flatnonzero(sdb.parent_vi == 0)
    for v in (int(sdb.species_vi[0]), int(genera[np.argmax(counts[genera])])):  # a leaf and the genus with the most k-mers
        p = tmp_path / f"v{v}.fastq"
        assert host.db2fastq(store, sdb.taxids, "proj", p, select=v, with_desc=False) == counts[v] > 0
        # (reader / writer test: the match result is not its subject; the double table is held to the oracle elsewhere)
        table, _, tot = host.match_files(store, [str(p)])
        assert table[v, 2] == table[v, 3] == counts[v]  # kmers, unique kmers
        assert tot.reads == counts[v]
    store.close()
