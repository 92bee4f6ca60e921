"""gs_dbupdate (the reference's updatedb stage, DBGoal.MyFastaReader, in its own streaming shape): a finished store on the device,
regions streamed past it in batches and slices, value := LCA(value, node of the region) per stored k-mer.  The expected arrays
come from the CPU restatement in stages (orc.DbBuild: fill, optimize, update any number of times), never from the library; the
one-shot device build of the same regions is a second witness.  Bit-exact arrays.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
import qualitycheck as qc
from genestrip_amd import synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

# T/tax/TaxTreeLCATest.java:51 plus value 7 without a tree node
PARENT = np.array([-1, 0, 1, 1, 2, 4, 0, -2], dtype=np.int32)
KS = (1, 2, 5, 16, 21, 31)
INVALID, UNSUPPORTED, STATE = -1, -4, -5


def _regions(k, step, seed, n=48):
    """-> (fill, update): lists of (bytes, node).  Noisy regions (lower case, N, CR, empty and tiny ones, a shared core, several
    regions per node); the update regions are the fill regions, more regions of other nodes over the same core, and regions the
    store has never seen"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    alphabet = np.frombuffer(b"ACGTacgtN\r", dtype=np.uint8)
    p = np.array([0.235, 0.235, 0.235, 0.235, 0.015, 0.015, 0.01, 0.01, 0.008, 0.002])
    core = rng.choice(acgt, 3000).tobytes()

    def noisy(r):
        body = bytearray(rng.choice(alphabet, int(rng.integers(0, 2500)), p=p).tobytes())
        if r % 2 == 0 and len(body) > 900:
            a = int(rng.integers(0, 2000))
            body[100:900] = core[a:a + 800]
        if r % 5 == 0:  # low-complexity islands for the DUST filter
            unit = rng.choice(acgt, int(rng.integers(1, 4))).tobytes()
            body += b"N" + (unit * 80)[:int(rng.integers(40, 160))] + rng.choice(acgt, 50).tobytes()
        return bytes(body), int(rng.integers(0, 7))

    fill = [noisy(r) for r in range(n)] + [(b"", 2), (b"ACGT" * 3, 5)]
    update = fill + [noisy(r) for r in range(n // 2)] + [(core, 6), (core[500:1500].lower(), 3), (b"", 1), (b"AC", 4)]
    return fill, update


def _batches(regions, n):
    cuts = np.linspace(0, len(regions), n + 1).astype(int)
    return [regions[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def _oracle(k, fill, update_batches, parent, lower=True, step=1, max_dust=-1):
    """-> (kmers, values after fill + optimize, values after every update batch)"""
    ob = orc.DbBuild(k, len(parent), parent, lower, step, max_dust)
    seq, off = qc.pack([s for s, _ in fill])
    ob.fill(seq, off, np.array([n for _, n in fill], dtype=np.int32))
    ob.optimize()
    kmers, before = ob.fetch()
    for part in update_batches:
        seq, off = qc.pack([s for s, _ in part])
        ob.update(seq, off, np.array([n for _, n in part], dtype=np.int32))
    k2, after = ob.fetch()
    ob.close()
    assert np.array_equal(kmers, k2)
    return kmers, before, after


def _device_fill(k, fill, parent, lower=True, step=1, max_dust=-1, update=(), close=True):
    gb = ga.DeviceDbBuilder(k, len(parent), parent, lower_case_bases=lower, step_size=step, max_dust=max_dust)
    seq, off = qc.pack([s for s, _ in fill])
    gb.add(seq, off, np.array([n for _, n in fill], dtype=np.int32), update=False)
    if update:
        seq, off = qc.pack([s for s, _ in update])
        gb.add(seq, off, np.array([n for _, n in update], dtype=np.int32), update=True)
    if not close:
        return gb
    out = gb.finish()
    gb.close()
    return out


def _add(u, part, device=False):
    seq, off = qc.pack([s for s, _ in part])
    nodes = np.array([n for _, n in part], dtype=np.int32)
    if device:
        import torch
        u.add(torch.from_numpy(seq.copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), nodes)
    else:
        u.add(seq, off, nodes)


def _stream(u, batches):
    """batches alternate between host arrays and device tensors -> (kmers, values, n_moved, stats)"""
    for i, part in enumerate(batches):
        _add(u, part, device=i % 2 == 1)
    moved = u.finish()
    kmers, vals = u.fetch()
    st = u.stats()
    u.close()
    return kmers, vals, moved, st


def _params(k, step):
    i = KS.index(k) * 3 + step
    return dict(lower=bool(i % 2), step=step, max_dust=(-1, k, k + 8)[i % 3])


@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("k", KS)
def test_streamed_update_equals_the_staged_reference(k, step):
    """cases 1, 6 and 7: builder over the fill regions -> fetch -> from_arrays -> the update regions as one batch, three batches
    and one region per call"""
    P = _params(k, step)
    fill, update = _regions(k, step, 1000 * k + step)
    wk, before, after = _oracle(k, fill, [update], PARENT, **P)
    assert len(wk) > (100 if k > 5 else 1)
    fk, fv = _device_fill(k, fill, PARENT, **P)
    assert np.array_equal(fk, wk) and np.array_equal(fv, before)
    assert k < 16 or (after != before).sum() > 100  # the update has work to do
    ok, ov = _device_fill(k, fill, PARENT, update=update, **P)  # the one-shot device build of the same regions
    assert np.array_equal(ok, wk) and np.array_equal(ov, after)
    want_moved = int((after != before).sum())
    for n_batches in (1, 3, len(update)):
        u = ga.DeviceDbUpdater.from_arrays(k, fk, fv, len(PARENT), PARENT, lower_case_bases=P["lower"], step_size=step, max_dust=P["max_dust"])
        gk, gv, moved, st = _stream(u, _batches(update, n_batches))
        assert np.array_equal(gk, wk), "the k-mer array must not change"
        assert np.array_equal(gv, after), (n_batches, int((gv != after).sum()))
        assert moved == want_moved and st.n_moved == want_moved and st.n_store == len(wk)
    # counters: every window of the update regions (the oracle's enumeration gives the distinct ones: the windows formed here in
    # numpy are held against it, and filtered by it when the DUST filter is on)
    distinct = qc.leaf_kmers(k, [s for s, _ in update], P["lower"], step, P["max_dust"])
    windows = _windows(k, [s for s, _ in update], P["lower"], step)
    if P["max_dust"] < 0:
        assert np.array_equal(np.unique(windows), distinct)
    else:
        assert np.isin(distinct, windows).all()
        windows = windows[np.isin(windows, distinct)]
    assert st.n_pairs == len(windows)
    assert st.n_found == int(np.isin(windows, wk).sum())


def _windows(k, regions, lower, step):
    """canonical k-mer of every window the reader forms (all of them, not the distinct ones): k bases in a row, taken when
    (bytes of the region so far) % step == 0; C G A T = 0 1 2 3, first base in the top bits, the larger strand"""
    code = np.full(256, 4, dtype=np.int64)
    for i, c in enumerate(b"CGAT"):
        code[c] = i
        if lower:
            code[c + 32] = i
    out = []
    w = (np.int64(1) << (2 * np.arange(k - 1, -1, -1, dtype=np.int64)))
    for s in regions:
        c = code[np.frombuffer(s, dtype=np.uint8)]
        if len(c) < k:
            continue
        win = np.lib.stride_tricks.sliding_window_view(c, k)
        start = np.arange(len(win))
        keep = (win < 4).all(axis=1) & ((start + k) % step == 0)
        win = win[keep]
        fwd = (win * w).sum(axis=1)
        rev = ((win ^ 1)[:, ::-1] * w).sum(axis=1)
        out.append(np.maximum(fwd, rev))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


@pytest.mark.parametrize("k,step", [(31, 1), (21, 2), (5, 3)])
def test_order_does_not_matter_and_twice_changes_nothing(k, step):
    P = _params(k, step)
    fill, update = _regions(k, step, 77 * k + step)
    wk, before, after = _oracle(k, fill, [update], PARENT, **P)
    fk, fv = _device_fill(k, fill, PARENT, **P)
    batches = _batches(update, 5)
    shuffled = [batches[i] for i in np.random.default_rng(5).permutation(len(batches))]
    results = []
    for order in (batches, batches[::-1], shuffled, [b for b in batches for _ in range(2)]):
        u = ga.DeviceDbUpdater.from_arrays(k, fk, fv, len(PARENT), PARENT, lower_case_bases=P["lower"], step_size=step, max_dust=P["max_dust"])
        gk, gv, moved, _ = _stream(u, order)
        results.append(moved)
        assert np.array_equal(gk, wk) and np.array_equal(gv, after)
    assert len(set(results)) == 1 and results[0] == int((after != before).sum())


@pytest.mark.parametrize("k,step", [(31, 1), (31, 3), (16, 1), (16, 3), (2, 1)])
def test_slices_do_not_change_the_result(k, step):
    """case 3: slices shorter than the longest region, and shorter than 2 k: regions are cut, no window is lost or formed twice"""
    P = _params(k, step)
    fill, update = _regions(k, step, 31 * k + step, n=24)
    longest = max(len(s) for s, _ in update)
    wk, before, after = _oracle(k, fill, [update], PARENT, **P)
    fk, fv = _device_fill(k, fill, PARENT, **P)
    ref = None
    for slice_bases in (None, longest // 3, max(2 * k - 1, k - 1 + step)):
        u = ga.DeviceDbUpdater.from_arrays(k, fk, fv, len(PARENT), PARENT, lower_case_bases=P["lower"], step_size=step, max_dust=P["max_dust"])
        if slice_bases:
            assert slice_bases < longest
            u.set_slice(slice_bases)
        gk, gv, moved, st = _stream(u, _batches(update, 2))
        assert np.array_equal(gk, wk) and np.array_equal(gv, after), slice_bases
        got = (moved, st.n_pairs, st.n_found)
        ref = ref or got
        assert got == ref, (slice_bases, got, ref)  # every window exactly once
    u = ga.DeviceDbUpdater.from_arrays(k, fk, fv, len(PARENT), PARENT, step_size=step)
    with pytest.raises(ga.GsError) as e:
        u.set_slice(k - 2 + step)
    assert e.value.code == INVALID
    u.close()


def _genome_case(seed=5):
    """genomes under root -> genus -> species.  Every genome is stored under its species (fill); U1 and U2 are the two halves
    of the collection in a shuffled order (U2 with two genomes of U1 again): they lift the shared k-mers"""
    db = synth.SynthDB(k=31, genera=3, species_per_genus=4, genome_len=40000, seed=seed)
    regions = [(bytes(g), int(v)) for g, v in zip(np.ascontiguousarray(db.genomes), db.species_vi)]
    shuffled = [regions[i] for i in np.random.default_rng(seed).permutation(len(regions))]
    half = len(shuffled) // 2
    return db, regions, shuffled[:half], shuffled[half:] + shuffled[:2]


def _match_equals_oracle(store, db, wk, wv, what):
    rs, ro = synth.reads_host(db.genomes, 4000, read_len=150, seed=9)
    m = ga.FastqKMerMatcher(store)
    cv, fl = m.match_reads(rs, ro.astype(np.uint64))
    table, dtable = m.finish()
    m.close()
    odb = orc.DB(31, wk, wv, db.n_values, db.parent_vi)
    o = matchcheck.oracle_batch(odb, rs, ro)
    matchcheck.check_match(o, dict(table=table, dtable=dtable, class_vi=cv, flags=fl), what)
    odb.close()


def test_an_existing_store_is_updated_after_save_and_load(tmp_path):
    """case 4: device build of fill + U1 -> store -> save -> load -> from_store -> U2 -> to_store; the arrays and a match equal the
    oracle's fill + U1 + U2"""
    db, fill, u1, u2 = _genome_case()
    wk, before, after = _oracle(31, fill, [u1, u2], db.parent_vi)
    _, _, mid = _oracle(31, fill, [u1], db.parent_vi)
    assert (after != mid).sum() > 100 and (mid != before).sum() > 100
    gb = _device_fill(31, fill, db.parent_vi, update=u1, close=False)
    built = gb.to_store()
    gb.close()
    path = str(tmp_path / "mid.gsstore")
    built.save(path)
    built.close()
    loaded = ga.DeviceKMerStore.load(path)
    u = ga.DeviceDbUpdater.from_store(loaded)
    loaded.close()  # the store is only read by from_store
    for part in _batches(u2, 3):
        _add(u, part)
    moved = u.finish()
    gk, gv = u.fetch()
    assert np.array_equal(gk, wk) and np.array_equal(gv, after)
    assert moved == int((after != mid).sum())
    store = u.to_store()
    u.close()
    assert store.info.n_stored == len(wk)
    ek, ev = store.export()
    assert np.array_equal(ek, wk) and np.array_equal(ev, after)
    _match_equals_oracle(store, db, wk, after, "updated store")
    store.close()


def test_a_partition_store_updates_its_part_and_a_stripe_is_refused():
    """case 4, partition store: each part is taken as the part it is; the parts' updated arrays together are the oracle's, and
    the store over them matches like the oracle.  (The parts go back into one plain store for the match: the split pipeline
    itself is the business of test_gpu_partitioned.py.)"""
    db, fill, u1, u2 = _genome_case(seed=8)
    wk, before, after = _oracle(31, fill, [u1, u2], db.parent_vi)
    _, _, mid = _oracle(31, fill, [u1], db.parent_vi)
    parts = []
    for part in range(2):
        ps = ga.DeviceKMerStore(31, wk, mid, db.n_values, db.parent_vi, n_parts=2, part=part, partition=True)
        pk, pv = ps.export()
        u = ga.DeviceDbUpdater.from_store(ps)
        ps.close()
        _add(u, u2)
        u.finish()
        gk, gv = u.fetch()
        u.close()
        assert 0 < len(pk) < len(wk) and np.array_equal(gk, pk)
        at = np.searchsorted(wk, gk)
        assert np.array_equal(wk[at], gk) and np.array_equal(gv, after[at]), part
        parts.append((gk, gv))
    keys = np.concatenate([p[0] for p in parts])
    vals = np.concatenate([p[1] for p in parts])
    o = np.argsort(keys)
    assert np.array_equal(keys[o], wk) and np.array_equal(vals[o], after)
    store = ga.DeviceKMerStore(31, keys[o], vals[o], db.n_values, db.parent_vi)
    _match_equals_oracle(store, db, wk, after, "updated partition stores")
    store.close()
    stripes = ga.DeviceKMerStore.striped(31, wk, mid, db.n_values, db.parent_vi, devices=(0, 0))
    with pytest.raises(ga.GsError) as e:
        ga.DeviceDbUpdater.from_store(stripes[0])
    assert e.value.code == UNSUPPORTED
    for s in stripes:
        s.close()


def test_from_builder_inherits_the_parameters_and_leaves_the_builder_alone():
    """case 5"""
    k, step = 21, 2
    P = _params(k, step)
    fill, update = _regions(k, step, 1000 * k + step)
    wk, before, after = _oracle(k, fill, [update], PARENT, **P)
    gb = _device_fill(k, fill, PARENT, close=False, **P)
    u = ga.DeviceDbUpdater.from_builder(gb)
    gk, gv, moved, _ = _stream(u, _batches(update, 3))
    assert np.array_equal(gk, wk) and np.array_equal(gv, after) and moved == int((after != before).sum())
    bk, bv = gb.finish()
    gb.close()
    assert np.array_equal(bk, wk) and np.array_equal(bv, before)
    unfinished = ga.DeviceDbBuilder(k, len(PARENT), PARENT)
    h = ga.binding.C.c_void_p()
    assert ga.lib().gs_dbupdate_begin_build(ga.binding.C.byref(h), unfinished.h) == STATE and not h.value
    unfinished.close()


def test_values_without_a_node_stay_and_the_kmers_never_change():
    """case 7: some stored k-mers carry value 7, which has no tree node: TaxTree.getLowestCommonAncestor answers null for it and
    the old value stays (DBGoal.java:246-251); every other k-mer is updated as if they were not there"""
    k, step = 31, 1
    fill, update = _regions(k, step, 4242)
    wk, before, after = _oracle(k, fill, [update], PARENT)
    changed = np.flatnonzero(after != before)
    assert len(changed) > 100
    orphan = np.concatenate([changed[::3], np.arange(0, len(wk), 7)])
    start = before.copy()
    start[orphan] = 7
    want = after.copy()
    want[orphan] = 7
    import torch
    u = ga.DeviceDbUpdater.from_arrays(k, torch.from_numpy(wk).cuda(), torch.from_numpy(start).cuda(), len(PARENT), PARENT)  # device arrays
    gk, gv, moved, _ = _stream(u, _batches(update, 2))
    assert np.array_equal(gk, wk) and np.array_equal(gv, want)
    assert moved == int((want != start).sum())


def test_refusals_leave_a_usable_handle():
    """case 8"""
    k, step = 16, 1
    fill, update = _regions(k, step, 99)
    wk, before, after = _oracle(k, fill, [update], PARENT)
    new = lambda kk=wk, vv=before, parent=PARENT: ga.DeviceDbUpdater.from_arrays(k, kk, vv, len(parent), parent)

    def code(fn):
        with pytest.raises(ga.GsError) as e:
            fn()
        return e.value.code

    u = new()
    seq, off = qc.pack([s for s, _ in update])
    nodes = np.array([n for _, n in update], dtype=np.int32)
    for bad in (9, -1, 7):  # out of range, negative, a value without a node
        b = nodes.copy()
        b[len(b) // 2] = bad
        assert code(lambda: u.add(seq, off, b)) == INVALID
    assert code(lambda: u.add(seq, off + np.uint64(1), nodes)) == INVALID  # offsets must start at 0
    assert u.stats().n_pairs == 0 and u.stats().n_moved == 0  # nothing happened
    assert code(u.fetch) == STATE and code(u.to_store) == STATE  # before finish
    u.add(seq, off, nodes)
    moved = u.finish()
    gk, gv = u.fetch()
    assert np.array_equal(gk, wk) and np.array_equal(gv, after) and moved == int((after != before).sum())
    assert code(lambda: u.add(seq, off, nodes)) == STATE
    assert u.finish() == moved  # a second finish repeats the count
    assert code(u.to_store) == UNSUPPORTED  # k = 16: a store without records, as gs_dbbuild_to_db
    u.close()
    assert code(lambda: new(parent=np.array([-1, 0, 1, 1, 2, 4, -1, -2], np.int32))) == UNSUPPORTED  # a forest
    swapped = wk.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    assert code(lambda: new(kk=swapped)) == INVALID
    dup = wk.copy()
    dup[20] = dup[19]
    assert code(lambda: new(kk=dup)) == INVALID
    beyond = wk.copy()
    beyond[-1] = np.int64(1) << 40  # still ascending, but not a k-mer of 16 bases
    assert code(lambda: new(kk=beyond)) == INVALID
    big = before.copy()
    big[3] = 8
    assert code(lambda: new(vv=big)) == INVALID
    empty = ga.DeviceDbUpdater.from_arrays(k, np.zeros(0, np.int64), np.zeros(0, np.int32), len(PARENT), PARENT)
    empty.add(seq, off, nodes)
    assert empty.finish() == 0 and empty.stats().n_found == 0 and empty.stats().n_pairs > 0
    assert len(empty.fetch()[0]) == 0
    empty.close()


def test_full_size_collection_streams_in_bounded_memory():
    """case 9: 500 genomes x 100 kbp (about 47 M k-mers).  The store is the device build of the fill regions; the update streams all
    genomes in batches of 50; the arrays equal the one-shot device build (itself pinned against the synthetic builder in
    test_gpu_build.py and here).  The working memory does not grow with the number of batches, and store + working memory stay
    below the one-shot builder's documented peak of 40 bytes per base of the collection."""
    import torch
    db = synth.SynthDB(k=31, genera=25, species_per_genus=20)
    g = db.genomes
    n_genomes, glen = g.shape
    assert n_genomes == 500 and glen == 100_000
    dseq = torch.from_numpy(np.ascontiguousarray(g).reshape(-1)).cuda()
    doff = torch.arange(n_genomes + 1, dtype=torch.int64, device="cuda") * glen
    one = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
    one.add(dseq, doff, db.species_vi, update=False)
    one.add(dseq, doff, db.species_vi, update=True)
    wk, wv = one.finish()
    one.close()
    assert np.array_equal(wk, db.kmers) and np.array_equal(wv, db.value_idx)
    gb = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
    gb.add(dseq, doff, db.species_vi, update=False)
    u = ga.DeviceDbUpdater.from_builder(gb)
    fk, fv = gb.finish()
    gb.close()
    assert np.array_equal(fk, wk)
    peaks = []
    boff = torch.arange(51, dtype=torch.int64, device="cuda") * glen
    for b in range(10):
        u.add(dseq[b * 50 * glen:(b + 1) * 50 * glen], boff, db.species_vi[b * 50:(b + 1) * 50])
        peaks.append(u.stats().batch_bytes_peak)
    moved = u.finish()
    st = u.stats()
    gk, gv = u.fetch()
    u.close()
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv)
    assert st.n_store == len(wk) and st.n_pairs == n_genomes * (glen - 30) and st.n_found == st.n_pairs
    assert moved == int((wv != fv).sum()) and moved > 0
    assert peaks[1] == peaks[9] and peaks[1] > 0, peaks
    assert st.batch_bytes_peak == peaks[9]
    assert st.store_bytes + st.batch_bytes_peak < 40 * n_genomes * glen, (st.store_bytes, st.batch_bytes_peak)
