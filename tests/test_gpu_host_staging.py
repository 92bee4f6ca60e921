"""Host batches (GS_MEM_HOST) are staged on the device by one piece of code for every entry point of the matcher and the filter,
and one handle's staging buffers are shared by its entry points.  One matcher and one filter live through batches that grow,
shrink, grow past the first capacity and shrink again, routed through every entry point in turn: a stale capacity, a wrong
rebase of a slice's offsets or an output copied from the wrong buffer shows against the oracle.  The kernel timer of both
handles counts exactly the profiled launches.  Needs an MI355X: run with -m gpu."""
import types

import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
from genestrip_amd import synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

K = 31
SIZES = (40, 1, 300, 7)  # grow, shrink, grow past the first capacity, shrink
CUTS = np.concatenate([[0], np.cumsum(SIZES)])  # batch i = reads [CUTS[i], CUTS[i + 1]): all but the first have offsets[0] != 0
N_READS = 400
FIXED_LEN = 150


@pytest.fixture(scope="module")
def world():
    sdb = synth.SynthDB(k=K, genera=2, species_per_genus=2, genome_len=5000, seed=7)
    rng = np.random.default_rng(41)
    g = sdb.genomes
    reads = []
    for i in range(N_READS):
        L = int(rng.integers(0, 401))
        if i in (3, 340):
            L = 0
        if i in (5, 40, 345):  # below k; read 40 is the batch of one
            L = int(rng.integers(1, K))
        p = int(rng.integers(0, g.shape[1] - L + 1))
        r = bytearray(g[int(rng.integers(0, g.shape[0]))][p:p + L].tobytes())
        if L and i % 23 == 0:
            r[int(rng.integers(0, L))] = ord("N")
        reads.append(bytes(r))
    seq, off = orc.pack_reads(reads)
    assert CUTS[-1] < N_READS and off[CUTS[1]] != 0
    fseq, foff = synth.reads_host(g, int(CUTS[-1]), read_len=FIXED_LEN, seed=19)
    text = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    odb = orc.DB(K, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    keys = sdb.kmers[np.isin(sdb.value_idx, sdb.species_vi)]
    ob = orc.Bloom(orc.BLOOM_XOR, len(keys), 1e-6)
    ob.put_many(keys)
    return types.SimpleNamespace(sdb=sdb, reads=reads, seq=seq, off=off, fseq=fseq, foff=foff.astype(np.uint64), text=text, odb=odb, ob=ob,
                                 accept=ob.filter_batch(K, 1, 0.2, seq, off))


def _sentinels(n):
    return np.full(n, -7, np.int32), np.full(n, 99, np.uint8)


def test_one_matcher_through_every_host_entry_point(world):
    w = world
    store = ga.DeviceKMerStore(K, w.sdb.kmers, w.sdb.value_idx, w.sdb.n_values, w.sdb.parent_vi)
    m = ga.FastqKMerMatcher(store, ga.MatchConfig(profile=True))
    fed = []  # (seq, offsets rebased to 0) of every batch that counts into the table, in read-number order
    got = []  # its per-read outputs
    launches = 0

    def feed(seq, offs):
        offs = np.asarray(offs, dtype=np.uint64)
        fed.append((seq[int(offs[0]):int(offs[-1])], offs - offs[0]))
        return sum(len(o) - 1 for _, o in fed[:-1])  # its first read number

    def check(cv, fl, what, i=-1):
        """a batch (the one fed last) against the oracle, as soon as its outputs are due: a later batch must not be able to mend it"""
        s, o = fed[i]
        ocv, ofl = orc.MatchRun(w.odb).submit(s if len(s) else np.zeros(1, np.uint8), o)
        assert np.array_equal(cv, ocv), (what, np.flatnonzero(cv != ocv)[:8])
        assert np.array_equal(fl, ofl), (what, np.flatnonzero(fl != ofl)[:8])
        got.append((cv, fl))

    # submit: slices of the big arrays
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        offs = w.off[a:b + 1]
        cv, fl = _sentinels(b - a)
        m.submit(w.seq, offs, feed(w.seq, offs), cv, fl)
        launches += 1
        check(cv, fl, f"submit [{a},{b})")

    # submit_fixed: reads of one length, no offsets
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        offs = w.foff[a:b + 1]
        cv, fl = _sentinels(b - a)
        m.submit_fixed(w.fseq[int(offs[0]):int(offs[-1])].copy(), FIXED_LEN, b - a, feed(w.fseq, offs), cv, fl)
        launches += 1
        check(cv, fl, f"submit_fixed [{a},{b})")

    # segments: the same staging, nothing into the table
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        seg_off, codes, _, lens = m.segments(w.seq, w.off[a:b + 1])
        for i in range(a, b):
            lo, hi = int(seg_off[i - a]), int(seg_off[i - a + 1])
            assert list(zip(codes[lo:hi].tolist(), lens[lo:hi].tolist())) == w.odb.segments(w.reads[i]), ("segments", a, b, i)

    # a text chunk with host outputs raises the shared per-read capacity (400 > 300) ...
    cv, fl = _sentinels(N_READS)
    first = feed(w.seq, w.off)
    m.submit_text(w.text, first_read_no=first, class_vi=cv, flags=fl)
    m.sync()
    launches += 1
    assert m.text_status()[0] == -1
    check(cv, fl, "submit_text")
    # ... and the host batch behind it, larger than every host batch before, trusts that capacity
    a, b = 20, 380
    offs = w.off[a:b + 1]
    cv, fl = _sentinels(b - a)
    m.submit(w.seq, offs, feed(w.seq, offs), cv, fl)
    launches += 1
    check(cv, fl, "submit behind the text chunk")

    # submit_async: two tickets under way, the second batch larger than the first; the third takes the first one's bank
    keep, tickets = [], []
    for a, b in ((0, 50), (50, 400), (33, 40)):
        offs = w.off[a:b + 1].copy()
        cv, fl = _sentinels(b - a)
        keep.append((offs, cv, fl))
        tickets.append(m.submit_async(w.seq, offs, feed(w.seq, offs), cv, fl))
        launches += 1
        if len(tickets) >= 2:
            m.wait(tickets[-2])
            check(keep[-2][1], keep[-2][2], f"submit_async {len(tickets) - 2}", -2)
    m.wait(tickets[-1])
    check(keep[-1][1], keep[-1][2], "submit_async 2")

    n1, ms1 = m.kernel_time()
    n2, ms2 = m.kernel_time()
    assert n1 == launches and ms1 > 0
    assert n2 == launches and ms2 == ms1  # collection empties the pending list

    table, dtable = m.finish()
    seq_all = np.concatenate([s for s, _ in fed])
    bases = np.concatenate([[0], np.cumsum([int(o[-1]) for _, o in fed])]).astype(np.uint64)
    off_all = np.concatenate([o[:-1] + base for (_, o), base in zip(fed, bases)] + [bases[-1:]])
    o = matchcheck.oracle_batch(w.odb, seq_all, off_all)
    matchcheck.check_match(o, dict(table=table, dtable=dtable, class_vi=np.concatenate([c for c, _ in got]),
                                   flags=np.concatenate([f for _, f in got])), "every host entry point")
    assert (o["flags"] & ga.F_FOUND).sum() > len(o["flags"]) // 2
    m.close()
    store.close()


def test_one_filter_through_every_host_entry_point(world):
    w = world
    gb = ga.DeviceBloomFilter(ga.BLOOM_XOR, w.ob.bits, w.ob.hash_factors, w.ob.words)
    f = ga.FastqBloomFilter(K, gb, 1, 0.2, profile=True)
    launches = 0
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        acc = np.full(b - a, 99, np.uint8)
        f.submit(w.seq, w.off[a:b + 1], acc)
        launches += 1
        assert np.array_equal(acc, w.accept[a:b]), ("submit", a, b, np.flatnonzero(acc != w.accept[a:b])[:8])
    acc = np.full(N_READS, 99, np.uint8)
    f.submit_text(w.text, acc)
    f.sync()
    launches += 1
    assert f.text_status()[0] == -1
    assert np.array_equal(acc, w.accept), ("submit_text", np.flatnonzero(acc != w.accept)[:8])
    a, b = 20, 380
    acc = np.full(b - a, 99, np.uint8)
    f.submit(w.seq, w.off[a:b + 1], acc)
    launches += 1
    assert np.array_equal(acc, w.accept[a:b]), ("submit behind the text chunk", np.flatnonzero(acc != w.accept[a:b])[:8])
    assert 0 < w.accept.sum() < N_READS
    n1, ms1 = f.kernel_time()
    n2, ms2 = f.kernel_time()
    assert n1 == launches and ms1 > 0
    assert n2 == launches and ms2 == ms1
    gb.close()
