"""Striped store (gs_db_create_striped / gs_db_create_stripe; VERDICT r01 "Next round" 4): ONE super-k-mer record table split
over the devices of a node, every device runs the ordinary fused kernel and loads foreign record lines over peer access.
On the one-GPU box every stripe lives on device 0 (a device may appear more than once), which exercises the stripe
arithmetic, the per-run seen bitmap, the merge and the finish with real kernels; what cannot be rehearsed here is only that
the pointers lead into another GPU's HBM.  Results must be bit-identical to the plain store and to the CPU oracle.
Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
from genestrip_amd import binding, synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sdb():
    return synth.SynthDB(k=31, genera=4, species_per_genus=4, genome_len=30000, seed=19)


@pytest.fixture(scope="module")
def reads(sdb):
    seq, off = synth.reads_host(sdb.genomes, 20000, read_len=150, seed=8)
    return seq, off.astype(np.uint64)


def _oracle_all(sdb, seq, off, **cfg):
    """the oracle's whole result for tests/matchcheck.py"""
    run = orc.MatchRun(orc.DB(sdb.k, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi), **cfg)
    cv, fl, terms = run.submit_terms(seq, off, 0, threads=8)
    t, d = run.finish()
    return dict(table=t, dtable=d, class_vi=cv, flags=fl, terms=terms)


@pytest.mark.parametrize("n_stripes", [2, 3, 5, 8])
@pytest.mark.parametrize("cfg", [{}, dict(count_unique=False, threshold=3), dict(max_paths=128)])
def test_one_run_on_a_striped_store_equals_the_oracle(sdb, reads, n_stripes, cfg):
    seq, off = reads
    o = _oracle_all(sdb, seq, off, **cfg)
    want = o["table"]
    stores = ga.DeviceKMerStore.striped(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, devices=(0,) * n_stripes)
    infos = [s.info for s in stores]
    assert [i.stripe for i in infos] == list(range(n_stripes)) and all(i.n_stripes == n_stripes for i in infos)
    assert sum(i.stripe_bytes for i in infos) == infos[0].rec_bytes + infos[0].table_bytes and infos[0].n_in_records > 0
    # any of the handles serves the whole store
    for s in (stores[0], stores[-1]):
        m = ga.FastqKMerMatcher(s, ga.MatchConfig(**cfg))
        cls, flags = m.match_reads(seq, off, 0)
        table, dtable = m.finish()
        assert np.array_equal(table, want), np.argwhere(table != want)[:6]
        # double sums: order dependent, held to the exact sum of their terms
        matchcheck.check_match(o, dict(table=table, dtable=dtable, class_vi=cls, flags=flags), f"{n_stripes} stripes")
        # a second batch after reset: the run's seen bits start from zero again
        m.reset()
        cls, flags = m.match_reads(seq[:int(off[500])], off[:501], 0)
        again, ad = m.finish()
        matchcheck.check_match(_oracle_all(sdb, seq[:int(off[500])], off[:501], **cfg),
                               dict(table=again, dtable=ad, class_vi=cls, flags=flags), "after reset")
        m.close()
    for s in stores:
        s.close()


def test_striped_runs_merge_like_replicas(sdb, reads):
    """one run per stripe handle (as with one GPU per stripe), each over its shard of the reads: gs_match_merge ORs the
    runs' seen bitmaps, and every run then holds the table of a single run over all reads"""
    seq, off = reads
    o = _oracle_all(sdb, seq, off)
    want = o["table"]
    stores = ga.DeviceKMerStore.striped(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, devices=(0, 0, 0))
    ms = [ga.FastqKMerMatcher(s) for s in stores]
    cuts = np.linspace(0, len(off) - 1, 4).astype(int)
    for m, a, b in zip(ms, cuts[:-1], cuts[1:]):
        m.submit(seq[int(off[a]):int(off[b])], off[a:b + 1] - off[a], int(a), n_reads=int(b - a))
    binding.merge_runs(ms)
    for i, m in enumerate(ms):
        t, d = m.finish()
        assert np.array_equal(t, want), np.argwhere(t != want)[:6]
        matchcheck.check_match(o, dict(table=t, dtable=d), f"stripe run {i}")
        m.close()
    for s in stores:
        s.close()


def test_files_over_the_handles_of_a_striped_store(sdb, tmp_path):
    """gs_host_match_files_multi (what a JVM host with one gs_run per GPU calls) takes the handles of ONE striped store just
    like replicas: files dealt to the handles, one thread each, merged, finished once"""
    from genestrip_amd import host
    seq, off = synth.reads_host(sdb.genomes, 9000, read_len=150, seed=77)
    off = off.astype(np.uint64)
    cuts = [0, 2500, 2501, 6000, 9000]
    paths = []
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        p = str(tmp_path / f"s{i}.fastq")
        with open(p, "wb") as f:
            for r in range(a, b):
                rd = seq[int(off[r]):int(off[r + 1])].tobytes()
                f.write(b"@r%d\n%s\n+\n%s\n" % (r, rd, b"F" * len(rd)))
        paths.append(p)
    o = _oracle_all(sdb, seq, off)
    want = o["table"]
    stores = ga.DeviceKMerStore.striped(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, devices=(0, 0, 0))
    table, dtable, tot = host.match_files_multi(stores, paths)
    assert tot.reads == 9000
    assert np.array_equal(table, want), np.argwhere(table != want)[:6]
    matchcheck.check_match(o, dict(table=table, dtable=dtable), "files over the stripe handles")
    single, sd, _ = host.match_files(stores[2], paths)
    assert np.array_equal(single, want)
    matchcheck.check_match(o, dict(table=single, dtable=sd), "files over one stripe handle")
    for s in stores:
        s.close()


def test_striped_store_long_reads_segments_and_max_counts(sdb):
    """the long-read kernel, the Kraken-style segments and the per-k-mer hit counters go through the stripes as well"""
    seq, off = synth.reads_host(sdb.genomes, 600, read_len=700, seed=31)
    off = off.astype(np.uint64)
    plain = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    stores = ga.DeviceKMerStore.striped(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, devices=(0, 0, 0, 0))
    cfg = ga.MatchConfig(max_kmer_res_counts=3)
    a, b = ga.FastqKMerMatcher(plain, cfg), ga.FastqKMerMatcher(stores[1], cfg)
    a.submit(seq, off, 0)
    b.submit(seq, off, 0)
    (ta, da), (tb, db_) = a.finish(), b.finish()
    assert np.array_equal(ta, tb) and ta[:, 2].sum() > 0
    o = _oracle_all(sdb, seq, off, max_kmer_res_counts=3)
    assert np.array_equal(ta, o["table"])
    assert np.array_equal(a.max_counts(), b.max_counts())
    mo = orc.MatchRun(orc.DB(sdb.k, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi), max_kmer_res_counts=3)
    mo.submit(seq, off, threads=8, per_read=False)
    o["max_counts"] = mo.max_counts()
    matchcheck.check_match(o, dict(table=ta, dtable=da, max_counts=a.max_counts()), "plain store")
    matchcheck.check_match(o, dict(table=tb, dtable=db_, max_counts=b.max_counts()), "4 stripes")
    sa, sb = a.segments(seq, off), b.segments(seq, off)
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    a.close(), b.close(), plain.close()
    for s in stores:
        s.close()


def test_a_store_file_loads_as_stripes(sdb, reads, tmp_path):
    """build once, save, load striped: the stripes of a store file serve the same tables as the store that was saved; a
    damaged file is refused before anything reaches HBM, as by gs_db_load"""
    seq, off = reads
    o = _oracle_all(sdb, seq, off)
    want = o["table"]
    plain = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    path = tmp_path / "store.gss"
    plain.save(path)
    pinfo = plain.info
    plain.close()
    stores = ga.DeviceKMerStore.load_striped(path, devices=(0, 0, 0, 0, 0))
    assert [s.info.stripe for s in stores] == [0, 1, 2, 3, 4] and stores[0].n_values == sdb.n_values and stores[0].k == 31
    assert stores[2].info.n_in_records == pinfo.n_in_records and stores[2].info.n_stored == pinfo.n_stored
    m = ga.FastqKMerMatcher(stores[3])
    m.submit(seq, off, 0)
    t, d = m.finish()
    assert np.array_equal(t, want), np.argwhere(t != want)[:6]
    matchcheck.check_match(o, dict(table=t, dtable=d), "stripes of a loaded file")
    m.close()
    for s in stores:
        s.close()
    one = ga.DeviceKMerStore.load_stripe(path, device=0, n_stripes=3, stripe=2)
    assert one.info.n_stripes == 3 and one.info.stripe == 2
    with pytest.raises(ga.GsError):
        ga.FastqKMerMatcher(one)  # the other stripes are not attached
    one.close()
    raw = bytearray(path.read_bytes())
    raw[len(raw) // 2] ^= 0x40
    bad = tmp_path / "bad.gss"
    bad.write_bytes(bytes(raw))
    with pytest.raises(ga.GsError) as e:
        ga.DeviceKMerStore.load_striped(bad, devices=(0, 0))
    assert e.value.code == -1 and "checksum" in str(e.value)


def test_striped_store_argument_errors(sdb):
    with pytest.raises(ga.GsError) as e:
        ga.DeviceKMerStore.striped(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, devices=(0,))
    assert e.value.code == -1
    with pytest.raises(ga.GsError):
        ga.DeviceKMerStore.striped(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, devices=(0,) * 9)
    with pytest.raises(ga.GsError):
        ga.DeviceKMerStore.striped(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, devices=(0, 99))
    small = synth.SynthDB(k=15, genera=2, species_per_genus=2, genome_len=3000, seed=2)
    with pytest.raises(ga.GsError) as e:  # k < 19: no records, nothing to stripe
        ga.DeviceKMerStore.striped(15, small.kmers, small.value_idx, small.n_values, small.parent_vi, devices=(0, 0))
    assert e.value.code == -4
    # one stripe of a multi-process store cannot serve a run before the others are attached, and is not a store file
    one = ga.DeviceKMerStore.stripe(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, device=0, n_stripes=2, stripe=1)
    with pytest.raises(ga.GsError) as e:
        ga.FastqKMerMatcher(one)
    assert e.value.code == -5
    with pytest.raises(ga.GsError):
        one.save("/tmp/never.gsstore")
    with pytest.raises(ga.GsError):
        one.attach_stripe(1, b"\0" * 64)  # its own stripe
    one.close()


def test_stripes_of_two_handles_attached_through_ipc_handles_in_one_process(sdb, reads):
    """gs_db_create_stripe + export / attach within one process is refused by HIP (an IPC handle cannot be opened by the
    process that made it), so here only the export side is exercised; the two-process case is tests/test_gpu_striped_mp"""
    one = ga.DeviceKMerStore.stripe(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi, device=0, n_stripes=2, stripe=0)
    h = one.export_stripe()
    assert len(h) == 64 and any(h)
    one.close()
