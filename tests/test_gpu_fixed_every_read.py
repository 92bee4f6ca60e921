"""What every read of a fixed-length batch executes in gs_match_kernel's FIXED loop, at the edges where it can go wrong.

The loop counts its trips down from a number worked out once per wave, writes its constant lane masks as literals, decides with one
test whether a read has per-read outputs at all, builds the base planes of a byte that is no upper-case CGAT letter from that byte's
own bits (only `bad` says that it is none) and sums the error count of a single-node read from scalar masks.  Every case here sends
the same reads through submit_fixed and through submit with an offsets array (the general loop) and holds both to the oracle with
tests/matchcheck.py: integer table, class_vi and flags bit for bit, every cell of the double table within its bound, and the two
double tables to each other by check_dtables_agree.  Reads as in tests/test_gpu_fixed_len.py: half from the genomes with 1 %
substitutions, half background.

  trip count        n_reads around the number of waves W of the launch (1, 2, W - 1, W, W + 1, 2 W + 3), at the default grid and at
                    GS_MATCH_BLOCKS_PER_CU=7 (another W), first_read_no 0 and 2^40 - 3 (the max key carries 40 bits of it)
  last read         a device buffer of exactly n_reads * L bytes, L = 128, 129, 150, 158: the third base word of the last read
  every byte value  0 .. 255 once in a genome read at base 0, 63, 64, 127, 128, max - 2, max - 1, max and L - 1, k = 31 and k = 23
  outputs           class_vi / flags null or given, on reads that only miss, only hit, and a mix with two-node reads
  neighbours        a store of more than 128 values (deferred records), threshold 2, both error gates
Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest
import torch

import genestrip_amd as ga
from genestrip_amd import synth
import matchcheck
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _reads(genomes, L, n, seed, background="odd", subs=0.01):
    """n reads of L bases back to back: windows of the genomes (synth.reads_host mixes background in by itself) with ~1 %
    substitutions; background = "odd": every second read is background, "all": every read, "none": no read"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, genomes.shape[0], n)
    p = rng.integers(0, genomes.shape[1] - L + 1, n)
    seq = np.ascontiguousarray(genomes[g[:, None], p[:, None] + np.arange(L)[None, :]], dtype=np.uint8)
    sub = rng.random((n, L)) < subs
    seq[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    if background == "odd":
        seq[1::2] = ACGT[rng.integers(0, 4, (len(seq[1::2]), L))]
    elif background == "all":
        seq[:] = ACGT[rng.integers(0, 4, (n, L))]
    return seq.reshape(-1)


def _oracle_low40(odb, seq, L, n, first, **cfg):
    """the oracle's result under the device's rule for MAX_CONTIG_READ_NO.  The max key of a row is (longest contig << 40 | 2^40 - 1 -
    low 40 bits of the read number): among the reads that tie on the longest contig the lowest number MODULO 2^40 wins, and that
    number is what the table shows.  The oracle keeps whole numbers.  A batch that crosses 2^40 therefore goes through ONE oracle run
    as two batches, each numbered by its low 40 bits (the oracle merges batches by the same rule: longest, then lowest number);
    every other column and the per-read outputs do not depend on the numbering.  Below 2^40 this is oracle_batch.
    The 40-bit key is the store's accumulator format, not something the FIXED loop brought: DESIGN.md section 3 (`max_keys`),
    gs_params.h (GsStatRec::max_key) and gs_match_finish, which gives the table the key's low 40 bits back.  Only
    MAX_CONTIG_READ_NO depends on it, and both submits, the general loop's included, are held to the same reference"""
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    cut = min(n, max(0, 2 ** 40 - first))  # reads [0, cut) have numbers below 2^40
    if cut == n:
        return matchcheck.oracle_batch(odb, seq, off, first_read_no=first, **cfg)
    run = orc.MatchRun(odb, **cfg)
    out = {}
    try:
        # (in the order of the low 40 bits: a thread of the oracle keeps the FIRST read it meets with the longest contig, which is the
        # lowest number only as long as the numbers it meets rise)
        for lo, hi, no in sorted(((0, cut, first), (cut, n, (first + cut) % 2 ** 40)), key=lambda p: p[2]):
            if hi > lo:
                out[lo] = run.submit_terms(seq[lo * L:hi * L], off[:hi - lo + 1], no, threads=8)
        t, d = run.finish()
    finally:
        run.close()
    cvs, fls, terms = zip(*(out[lo] for lo in sorted(out)))  # back in read order
    return dict(table=t, dtable=d, class_vi=np.concatenate(cvs), flags=np.concatenate(fls), terms=np.concatenate(terms))


class _Case:
    """one store with its oracle; check() runs one batch through both submits and the oracle"""

    def __init__(self, db, k=None):
        self.db, self.k = db, (k or db.k)
        self.odb = orc.DB(self.k, db.kmers, db.value_idx, db.n_values, db.parent_vi)
        self.store = ga.DeviceKMerStore(self.k, db.kmers, db.value_idx, db.n_values, db.parent_vi)

    def close(self):
        self.store.close()

    def check(self, seq, L, n, what, first=0, want_cv=True, want_fl=True, device=False, **cfg):
        seq = np.ascontiguousarray(seq[:n * L])
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
        o = _oracle_low40(self.odb, seq, L, n, first, **cfg)
        m = ga.FastqKMerMatcher(self.store, ga.MatchConfig(**cfg))
        try:
            res = []
            for fixed in (False, True):
                m.reset()
                cv = np.full(n, -7, dtype=np.int32) if want_cv else None
                fl = np.full(n, 0xee, dtype=np.uint8) if want_fl else None
                if device:  # a buffer of exactly n * L bytes on the device
                    dseq = torch.from_numpy(seq).cuda()
                    assert dseq.numel() == n * L
                    dcv = torch.from_numpy(cv).cuda() if want_cv else None
                    dfl = torch.from_numpy(fl).cuda() if want_fl else None
                    if fixed:
                        m.submit_fixed(dseq, L, n, first, class_vi=dcv, flags=dfl)
                    else:
                        m.submit(dseq, torch.from_numpy(off.view(np.int64)).cuda(), first, class_vi=dcv, flags=dfl, n_reads=n)
                    m.sync()
                    cv = dcv.cpu().numpy() if want_cv else None
                    fl = dfl.cpu().numpy() if want_fl else None
                elif fixed:
                    m.submit_fixed(seq, L, n, first, class_vi=cv, flags=fl)
                else:
                    m.submit(seq, off, first, class_vi=cv, flags=fl)
                t, d = m.finish()
                res.append(dict(table=t, dtable=d, class_vi=cv, flags=fl))
        finally:
            m.close()
        a, f = res
        matchcheck.check_match(o, a, what + " offsets array")
        matchcheck.check_match(o, f, what + " fixed")
        assert np.array_equal(f["table"], a["table"]), what + ": tables of the two submits differ"
        if want_cv:
            assert np.array_equal(f["class_vi"], a["class_vi"]), what + ": class_vi of the two submits differs"
        if want_fl:
            assert np.array_equal(f["flags"], a["flags"]), what + ": flags of the two submits differ"
        matchcheck.check_dtables_agree(f["dtable"], a["dtable"], a["table"][:, orc.C_READS], what + ": double tables of the two submits")
        return o


@pytest.fixture(scope="module")
def db31():
    return synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)


@pytest.fixture(scope="module")
def case31(db31):
    c = _Case(db31)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case23():
    c = _Case(synth.SynthDB(k=23, genera=3, species_per_genus=3, genome_len=20000, seed=11))
    yield c
    c.close()


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- trip count -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trip_reads(db31):
    n = 2 * 32 * _n_cu() + 3
    return _reads(db31.genomes, 150, n, seed=31150)


@pytest.mark.parametrize("first", [0, 2 ** 40 - 3], ids=["first0", "first2p40m3"])
@pytest.mark.parametrize("blocks", [None, 7], ids=["grid_default", "grid_7_per_cu"])
def test_trip_count_around_the_number_of_waves(db31, trip_reads, monkeypatch, blocks, first):
    """W waves take reads w, w + W, ...: n_reads of 1, 2, W - 1, W, W + 1 and 2 W + 3 give waves of 0, 1, 2 and 3 trips, and the last
    wave with a read is the first, the second, the last but one and the last of the grid"""
    if blocks is None:
        monkeypatch.delenv("GS_MATCH_BLOCKS_PER_CU", raising=False)
    else:
        monkeypatch.setenv("GS_MATCH_BLOCKS_PER_CU", str(blocks))
    per_cu = 8 if blocks is None else blocks
    W = 4 * per_cu * _n_cu()
    case = _Case(db31)  # (the grid is fixed when a matcher begins: check() begins one per batch, under this environment)
    try:
        hits = 0
        for n in (1, 2, W - 1, W, W + 1, 2 * W + 3):
            assert n * 150 <= len(trip_reads)
            o = case.check(trip_reads, 150, n, f"{per_cu} blocks per CU, first {first}, n_reads {n}", first=first)
            hits += int(np.count_nonzero(o["flags"] & orc.F_FOUND))
            if n >= W - 1:  # the table's read numbers are low 40 bits of numbers of this batch; above 2^40 - 3 + 2 they have wrapped
                t = o["table"]
                no = t[t[:, orc.C_MAX_CONTIG_LEN] > 0, orc.C_MAX_CONTIG_READ_NO]
                assert len(no) and np.all(((no >= first) & (no < min(first + n, 2 ** 40))) | ((no >= 0) & (no < first + n - 2 ** 40)))
                assert first == 0 or np.any(no < n)
        assert hits > W
    finally:
        case.close()


# ---- last read of the buffer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [128, 129, 150, 158])
def test_last_read_of_an_exact_device_buffer(case31, db31, L):
    """the sequence tensor holds n_reads * L bytes and not one more: the third base word of the last read (bases 128 .. L - 1, none at
    L = 128) comes from inside the read.  An odd n makes the last read a genome read"""
    n = 2001
    seq = _reads(db31.genomes, L, n, seed=7000 + L)
    o = case31.check(seq, L, n, f"exact buffer L {L}", device=True)
    assert o["flags"][n - 1] & orc.F_FOUND


# ---- every byte value -------------------------------------------------------------------------------------------------------------
def _byte_positions(L, k):
    mx = L - k + 1
    return sorted({0, 63, 64, 127, 128, mx - 2, mx - 1, mx, L - 1})  # (k = 23: max = 128, two of them coincide)


@pytest.mark.parametrize("k", [31, 23])
def test_every_byte_value_at_the_word_and_census_edges(case31, case23, k):
    """read 256 p + b is a clean genome read with byte value b at position p: 253 of the 256 values are no upper-case CGAT letter and
    make every window over them invalid (and count as an error where the census counts them); 'C', 'G', 'A' and 'T' are a base.
    The planes the FIXED loop builds for the 252 others differ from the general loop's; no result may"""
    case = case31 if k == 31 else case23
    L = 150
    pos = _byte_positions(L, k)
    assert all(0 <= p < L for p in pos)
    n = 256 * len(pos)
    seq = _reads(case.db.genomes, L, n, seed=900 + k, background="none", subs=0.0).reshape(n, L)
    for i, p in enumerate(pos):
        seq[256 * i:256 * (i + 1), p] = np.arange(256, dtype=np.uint8)
    cfgs = [dict(), dict(max_read_tax_err=0.1, max_read_class_err=0.5)]
    for cfg in cfgs:
        o = case.check(seq.reshape(-1), L, n, f"k {k} byte values {cfg}", **cfg)
        found = (o["flags"] & orc.F_FOUND) != 0
        assert found.sum() > n // 2  # (an invalid window takes k positions of ~120 away: the reads still hit)


# ---- per-read outputs null or given -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def output_batches(db31):
    n = 3000
    return {kind: _reads(db31.genomes, 150, n, seed=5000 + i, background=bg)
            for i, (kind, bg) in enumerate([("miss", "all"), ("hit", "none"), ("mix", "odd")])}, n


@pytest.mark.parametrize("want_fl", [False, True], ids=["no_flags", "flags"])
@pytest.mark.parametrize("want_cv", [False, True], ids=["no_class_vi", "class_vi"])
@pytest.mark.parametrize("kind", ["miss", "hit", "mix"])
def test_outputs_null_or_given(case31, output_batches, kind, want_cv, want_fl):
    """the store holds genus and root k-mers next to the species': the mix (and the hit batch) has reads of two nodes, which take the
    lane-parallel booking, next to reads of one, which take the scalar one, next to reads of none"""
    batches, n = output_batches
    o = case31.check(batches[kind], 150, n, f"{kind} class_vi {want_cv} flags {want_fl}", want_cv=want_cv, want_fl=want_fl)
    found = int(np.count_nonzero(o["flags"] & orc.F_FOUND))
    pairs = int(o["table"][:, orc.C_READS_1KMER].sum())  # (read, tax id) pairs
    if kind == "miss":
        assert found == 0 and np.all(o["class_vi"] == -1)
    if kind == "hit":
        assert found > n - n // 20
    if kind == "mix":
        assert n // 3 < found < n - n // 3 and pairs > found  # some reads have two nodes


# ---- neighbours of the changed paths ----------------------------------------------------------------------------------------------
def test_store_above_lds_statistics_with_gates():
    """more than 128 values: counters in global memory, reads of one tax id deferred into records; both error gates on, at
    threshold 1 and at threshold 2"""
    db = synth.SynthDB(k=31, genera=13, species_per_genus=10, genome_len=4000, seed=5)
    assert db.n_values > 128
    case = _Case(db)
    try:
        seq = _reads(db.genomes, 150, 3001, seed=77)
        o = case.check(seq, 150, 3001, "deferred records, gates", max_read_tax_err=0.1, max_read_class_err=0.5)
        assert 0 < int(o["table"][:, orc.C_READS].sum()) < int(np.count_nonzero(o["flags"] & orc.F_FOUND))
        case.check(seq, 150, 3001, "deferred records, no outputs", want_cv=False, want_fl=False)
        o = case.check(seq, 150, 3001, "deferred records, threshold 2, gates", threshold=2, max_read_tax_err=0.1, max_read_class_err=0.5)
        assert 0 < int(o["table"][:, orc.C_READS].sum())
    finally:
        case.close()


def test_threshold_two_with_gates(case31, db31):
    seq = _reads(db31.genomes, 150, 3001, seed=78)
    o = case31.check(seq, 150, 3001, "threshold 2, gates", threshold=2, max_read_tax_err=0.1, max_read_class_err=0.5)
    assert 0 < int(o["table"][:, orc.C_READS].sum())
