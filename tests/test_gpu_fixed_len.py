"""gs_match_submit_fixed against gs_match_submit at EVERY read length the short-read kernel can meet.

A batch of one read length is matched by a loop of gs_match_kernel that settles per wave, not per read, what the length alone
decides (lengths of 128 .. k + 127 bases; gs_kernels.hip "pays for its length once"); every other length, and every batch with an
offsets array, takes the general loop.  For every length from k - 1 (no k-mer) over k (one k-mer) to k + 127 (128 positions), at
k = 31 (k folded in at compile time) and k = 23 (any-k kernels), the same reads go through submit_fixed and through submit with an
offsets array: integer table, class_vi and flags must be equal to each other and to the oracle bit for bit.  The double table of
each is held to the oracle by tests/matchcheck.py (every cell within (n + 3) * 2^-53 of the exact sum of its terms) and the two to
each other by matchcheck.check_dtables_agree: the order of a double sum is the device's from launch to launch, so two launches of
the SAME code need not agree in the last bits, and that bound is what "equal" means for these columns throughout the suite.

Reads: half from the store's genomes with substitutions, half background; some with an N at the first, the last and a middle
position, some with one lower-case base.  Two more cases walk the reduce with the hoisted masks on other paths: a store of more than
128 values (counters in global memory, deferred records) and a threshold above 1.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import genestrip_amd as ga
from genestrip_amd import synth
import matchcheck
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

N_READS = 2000


def _reads(db, L, n, seed):
    """n reads of L bases back to back: even reads from the genomes with ~1 % substitutions, odd reads background"""
    rng = np.random.default_rng(seed)
    seq, off = synth.reads_host(db.genomes, n, read_len=L, seed=seed)
    seq = seq.copy().reshape(n, L)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    sub = rng.random((n, L)) < 0.01
    seq[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    seq[1::2] = acgt[rng.integers(0, 4, (n // 2, L))]
    # non-CGAT bytes: an N at the first / the last / a middle position, one lower-case base (rows of both halves)
    seq[10::40, 0] = ord("N")
    seq[11::40, L - 1] = ord("N")
    seq[12::40, L // 2] = ord("N")
    seq[13::40, 0] = ord("N")
    seq[13::40, L - 1] = ord("N")
    rows = np.arange(14, n, 40)
    cols = rng.integers(0, L, len(rows))
    seq[rows, cols] |= 0x20
    return seq.reshape(-1), off


def _compare(db, k, lengths, n=N_READS, **cfg):
    odb = orc.DB(k, db.kmers, db.value_idx, db.n_values, db.parent_vi)
    store = ga.DeviceKMerStore(k, db.kmers, db.value_idx, db.n_values, db.parent_vi)
    m = ga.FastqKMerMatcher(store, ga.MatchConfig(**cfg))
    failures = []
    hits = 0
    for L in lengths:
        seq, off = _reads(db, L, n, seed=1000 * k + L)
        assert np.array_equal(off, np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
        try:
            o = matchcheck.oracle_batch(odb, seq, off, **cfg)
            m.reset()
            cv_a, fl_a = m.match_reads(seq, off)
            t_a, d_a = m.finish()
            m.reset()
            cv_f, fl_f = np.full(n, -7, dtype=np.int32), np.full(n, 0xee, dtype=np.uint8)
            m.submit_fixed(seq, L, n, class_vi=cv_f, flags=fl_f)
            t_f, d_f = m.finish()
            matchcheck.check_match(o, dict(table=t_a, dtable=d_a, class_vi=cv_a, flags=fl_a), f"k {k} L {L} offsets array")
            matchcheck.check_match(o, dict(table=t_f, dtable=d_f, class_vi=cv_f, flags=fl_f), f"k {k} L {L} fixed")
            assert np.array_equal(t_f, t_a), f"k {k} L {L}: tables of the two submits differ"
            assert np.array_equal(cv_f, cv_a) and np.array_equal(fl_f, fl_a), f"k {k} L {L}: per-read outputs of the two submits differ"
            matchcheck.check_dtables_agree(d_f, d_a, t_a[:, orc.C_READS], f"k {k} L {L}: double tables of the two submits")
            hits += int((fl_f & 1).sum())
            if L < k:
                assert not fl_f.any() and np.all(cv_f == -1), f"k {k} L {L}: a read without a k-mer matched"
        except AssertionError as e:
            failures.append(str(e)[:400])
    m.close()
    store.close()
    assert not failures, f"{len(failures)} lengths fail, first: {failures[:3]}"
    return hits


@pytest.fixture(scope="module", params=[31, 23], ids=["k31", "k23"])
def kdb(request):
    return synth.SynthDB(k=request.param, genera=3, species_per_genus=3, genome_len=20000, seed=11)


def test_every_length_fixed_equals_offsets_equals_oracle(kdb):
    """every length from k - 1 (no k-mer) and k (one k-mer) to k + 127 (128 positions): 129 lengths, none left out"""
    k = kdb.k
    lengths = list(range(k - 1, k + 128))
    assert len(lengths) == 129 and lengths[0] == k - 1 and lengths[-1] - k + 1 == 128
    hits = _compare(kdb, k, lengths)
    assert hits > 100 * len(lengths)  # (the genome half of the reads does hit the store)


def test_store_above_lds_statistics():
    """more than 128 values: counters in global memory, reads of one tax id deferred into records (the !LDS_STATS instantiation)"""
    db = synth.SynthDB(k=31, genera=13, species_per_genus=10, genome_len=4000, seed=5)
    assert db.n_values > 128
    assert _compare(db, 31, [30, 31, 100, 127, 128, 129, 150, 157, 158]) > 0


def test_threshold_above_one(kdb):
    """threshold > 1: the distinct-node list goes through LDS and the class needs enough votes"""
    k = kdb.k
    assert _compare(kdb, k, [k - 1, k, k + 3, 127, 128, 129, 150, k + 126, k + 127], threshold=4, max_paths=3) > 0
