"""gs_dbbuild (VERDICT r01 "what's missing" 6): the compute core of FillDBGoal + DBGoal on the device --
k-mers of genome regions, one radix sort, LCA fold per distinct k-mer -- against the CPU restatement (orc_build_*), against
the synthetic store builder (numpy, an independent third implementation of "LCA of all genomes that hold the k-mer"), and
through to a match on the store it produced.  Bit-exact arrays.  Needs an MI355X: run with -m gpu."""
import os

import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
from genestrip_amd import synth
from conftest import GOLDEN
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

PARENT = np.array([-1, 0, 1, 1, 2, 4, 0], dtype=np.int32)  # T/tax/TaxTreeLCATest.java:51


def _pack(parts):
    seq = np.frombuffer(b"".join(parts), dtype=np.uint8)
    if len(seq) == 0:
        seq = np.zeros(1, dtype=np.uint8)
    return seq, np.cumsum([0] + [len(s) for s in parts]).astype(np.uint64)


def _both(k, fill, update, parent, lower=True, step=1, batches=1, max_dust=-1):
    """fill / update: lists of (bytes, node).  -> (device arrays, oracle arrays)"""
    ob = orc.DbBuild(k, len(parent), parent, lower, step, max_dust)
    gb = ga.DeviceDbBuilder(k, len(parent), parent, lower_case_bases=lower, step_size=step, max_dust=max_dust)
    for upd, regions in ((False, fill), (True, update)):
        if upd:
            ob.optimize()
        cuts = np.linspace(0, len(regions), batches + 1).astype(int)
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = regions[a:b]
            if not part:
                continue
            seq, off = _pack([s for s, _ in part])
            nodes = np.array([n for _, n in part], dtype=np.int32)
            (ob.update if upd else ob.fill)(seq, off, nodes)
            gb.add(seq, off, nodes, update=upd)
    if not update:
        ob.optimize()
    want = ob.fetch()
    got = gb.finish()
    ob.close()
    gb.close()
    return got, want


@pytest.mark.parametrize("k,lower,step,batches", [(31, True, 1, 1), (31, True, 1, 3), (21, False, 1, 2), (5, True, 3, 1), (1, True, 1, 1), (19, True, 2, 4)])
def test_device_build_equals_the_restatement_on_noisy_regions(k, lower, step, batches):
    rng = np.random.default_rng(1000 * k + step)
    alphabet = np.frombuffer(b"ACGTacgtN\r", dtype=np.uint8)
    p = np.array([0.235, 0.235, 0.235, 0.235, 0.015, 0.015, 0.01, 0.01, 0.008, 0.002])
    core = rng.choice(alphabet[:4], 3000).tobytes()
    fill = []
    for r in range(60):
        body = bytearray(rng.choice(alphabet, int(rng.integers(0, 2500)), p=p).tobytes())
        if r % 2 == 0 and len(body) > 900:
            a = int(rng.integers(0, 2000))
            body[100:900] = core[a:a + 800]
        fill.append((bytes(body), int(rng.integers(0, 7))))
    fill += [(b"", 2), (b"ACGT" * 3, 5)]
    update = fill + [(core, 6), (core[500:1500].lower(), 3)]
    (gk, gv), (wk, wv) = _both(k, fill, update, PARENT, lower, step, batches)
    assert len(wk) > (100 if k > 2 else 1)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv), (len(gk), len(wk))
    # fill only (no DBGoal pass): the first region's node stays
    (gk, gv), (wk, wv) = _both(k, fill, [], PARENT, lower, step, batches)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv)


@pytest.mark.parametrize("k,max_dust", [(31, 0), (31, 20), (31, 500), (21, 8), (5, 2), (3, 1)])
def test_low_complexity_filter_on_the_device(k, max_dust):
    """maxDust: k-mers whose score (sum of fib(run length) over the runs of period 1, 2, 3) exceeds it are skipped in both passes;
    the device scores a k-mer from its planes, the restatement streams like CGATLongBuffer"""
    rng = np.random.default_rng(7 * k + max_dust)
    fill = []
    for r in range(40):
        parts = []
        for _ in range(12):
            parts.append(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(rng.integers(1, 120))).tobytes())
            unit = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(rng.integers(1, 4))).tobytes()
            parts.append((unit * 60)[:int(rng.integers(0, 90))])
            if rng.random() < 0.2:
                parts.append(b"N")
        fill.append((b"".join(parts), int(rng.integers(0, 7))))
    (gk, gv), (wk, wv) = _both(k, fill, fill[::2], PARENT, True, 1, 2, max_dust)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv), (len(gk), len(wk))
    (nk, _), _ = _both(k, fill, [], PARENT, True, 1, 1, -1)
    assert len(gk) < len(nk)  # the filter took something out


def test_device_build_reproduces_the_synthetic_store_and_serves_a_match():
    """the bench's store recipe (genomes under a root -> genus -> species tree, value = LCA of all genomes that hold the
    k-mer) from its genomes alone, then reads against the store built from the device's arrays"""
    db = synth.SynthDB(k=31, genera=3, species_per_genus=4, genome_len=40000, seed=5)
    genomes = db.genomes
    seq = np.ascontiguousarray(genomes).reshape(-1)
    off = (np.arange(genomes.shape[0] + 1) * genomes.shape[1]).astype(np.uint64)
    gb = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
    gb.add(seq, off, db.species_vi, update=False)
    gb.add(seq, off, db.species_vi, update=True)
    keys, vals = gb.finish()
    gb.close()
    assert np.array_equal(keys, db.kmers) and np.array_equal(vals, db.value_idx)
    store = ga.DeviceKMerStore(31, keys, vals, db.n_values, db.parent_vi)
    rs, ro = synth.reads_host(genomes, 4000, read_len=150, seed=9)
    m = ga.FastqKMerMatcher(store)
    m.submit(rs, ro.astype(np.uint64), 0)
    table, dtable = m.finish()
    odb = orc.DB(31, db.kmers, db.value_idx, db.n_values, db.parent_vi)
    o = matchcheck.oracle_batch(odb, rs, ro)
    assert np.array_equal(table, o["table"])
    matchcheck.check_match(o, dict(table=table, dtable=dtable), "device-built arrays")
    m.close(), store.close(), odb.close()


def test_genomes_to_store_without_leaving_the_device():
    """gs_dbbuild_to_db: genomes -> (k-mer, LCA) arrays -> store layout, all on the GPU; the store answers like one built from the
    host recipe's arrays, and its file loads"""
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
    assert store.info.n_stored == len(db.kmers) and store.info.n_in_records > 0.9 * len(db.kmers)
    rs, ro = synth.reads_host(g, 4000, read_len=150, seed=9)
    m = ga.FastqKMerMatcher(store)
    m.submit(rs, ro.astype(np.uint64), 0)
    table, dtable = m.finish()
    m.close()
    odb = orc.DB(31, db.kmers, db.value_idx, db.n_values, db.parent_vi)
    o = matchcheck.oracle_batch(odb, rs, ro)
    assert np.array_equal(table, o["table"])
    matchcheck.check_match(o, dict(table=table, dtable=dtable), "device-built store")
    odb.close()
    store.close()


def test_build_in_kmer_ranges_equals_one_build():
    """a collection too big for one pass: one builder per range of the canonical k-mer, results one behind the other"""
    from genestrip_amd.binding import kmer_ranges
    db = synth.SynthDB(k=31, genera=2, species_per_genus=3, genome_len=30000, seed=12)
    g = db.genomes
    seq = np.ascontiguousarray(g).reshape(-1)
    off = (np.arange(g.shape[0] + 1) * g.shape[1]).astype(np.uint64)
    ranges = kmer_ranges(31, 5)
    assert ranges[0][0] == 0 and ranges[-1][1] == 1 << 62 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    parts, sizes = [], []
    for lo, hi in ranges:
        b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
        b.set_range(lo, hi)
        b.add(seq, off, db.species_vi, update=False)
        b.add(seq, off, db.species_vi, update=True)
        k, v = b.finish()
        assert len(k) == 0 or (k[0] >= lo and k[-1] < hi)
        parts.append((k, v))
        sizes.append(len(k))
        with pytest.raises(ga.GsError):
            b.set_range(0, 5)  # only before the first add
        b.close()
    keys = np.concatenate([p[0] for p in parts])
    vals = np.concatenate([p[1] for p in parts])
    assert np.array_equal(keys, db.kmers) and np.array_equal(vals, db.value_idx)
    assert max(sizes) < 1.25 * min(sizes)  # the ranges are balanced


def test_device_build_from_device_memory_and_the_dengue_fixture():
    import torch
    raw = open(os.path.join(GOLDEN, "dengue1", "dengue1.fasta"), "rb").read()
    rd = orc.parse_fastq(raw, fasta=True, k=31)
    dseq = torch.from_numpy(np.ascontiguousarray(rd["seq"])).cuda()
    doff = torch.from_numpy(rd["seq_off"].astype(np.int64)).cuda()
    gb = ga.DeviceDbBuilder(31, 1, np.array([-1], np.int32))
    gb.add(dseq, doff, np.array([0], np.int32))
    keys, vals = gb.finish()
    gb.close()
    want = np.unique(orc.canonical_kmers(bytes(rd["seq"]).decode().upper(), 31))
    assert np.array_equal(keys, want) and not vals.any()


def test_device_build_argument_errors():
    with pytest.raises(ga.GsError) as e:
        ga.DeviceDbBuilder(31, 7, PARENT, max_dust=40000)  # beyond Short.MAX_VALUE: the reference refuses it too
    assert e.value.code == -1
    with pytest.raises(ga.GsError) as e:
        ga.DeviceDbBuilder(31, 3, np.array([-1, -1, 0], np.int32))  # two roots
    assert e.value.code == -4
    with pytest.raises(ga.GsError):
        ga.DeviceDbBuilder(32, 7, PARENT)
    with pytest.raises(ga.GsError):
        ga.DeviceDbBuilder(31, 3, np.array([-1, 2, 1], np.int32))  # a cycle
    b = ga.DeviceDbBuilder(5, 7, PARENT)
    seq, off = _pack([b"ACGTACGT"])
    with pytest.raises(ga.GsError):
        b.add(seq, off, np.array([9], np.int32))  # not a node
    with pytest.raises(ga.GsError):
        b.add(seq, np.array([1, 8], np.uint64), np.array([0], np.int32))  # offsets must start at 0
    b.add(seq, off, np.array([3], np.int32))
    keys, vals = b.finish()
    assert len(keys) == len(np.unique(orc.canonical_kmers("ACGTACGT", 5))) and (vals == 3).all()
    with pytest.raises(ga.GsError) as e:
        b.add(seq, off, np.array([3], np.int32))
    assert e.value.code == -5
    b.close()
    empty = ga.DeviceDbBuilder(5, 7, PARENT)
    k0, v0 = empty.finish()
    assert len(k0) == 0 and len(v0) == 0
    empty.close()


@pytest.mark.parametrize("kind", [orc.BLOOM_XOR, orc.BLOOM_MURMUR])
@pytest.mark.parametrize("n,fpp", [(5000, 1e-8), (200000, 0.01), (1, 1e-8), (37, 0.5)])
def test_index_filter_built_on_the_device_equals_the_reference_construction(n, fpp, kind):
    """gs_bloom_build (BloomIndexGoal): geometry, hash factors and every bit equal the oracle's XOR filter after putLong of the
    same k-mers; a filter goal on it accepts what the oracle's accepts"""
    rng = np.random.default_rng(n)
    keys = np.unique(rng.integers(0, 1 << 62, n, dtype=np.int64))
    ob = orc.Bloom(kind, len(keys), fpp)
    ob.put_many(keys)
    f = ga.DeviceBloomFilter.build(keys, fpp=fpp, kind=kind)
    bits, hf, words = f.get()
    assert bits == ob.bits and len(hf) == ob.hashes and np.array_equal(hf, ob.hash_factors)
    assert np.array_equal(words, ob.words[:len(words)])
    if n >= 5000:  # the filter goal over it
        import torch
        g = ga.DeviceBloomFilter.build(torch.from_numpy(keys).cuda(), fpp=fpp, kind=kind)  # the same from device memory
        assert np.array_equal(g.get()[2], words)
        g.close()
    f.close()
    ob.close()
