"""gs_pf_kernel at the sizes where its paths change (genestrip_amd/csrc/gs_prefilter.hip), every case through tests/test_gpu_prefilter.py's
_check: prefilter forced on, forced off and the CPU oracle agree in every output, and the survivors are exactly those of
tests/prefilter.py; the sample counts also with the kernel launched on its own (gs_launch_prefilter), which reaches the lengths
below 128 that the library does not prefilter.  Batch sizes around a wave round and a workgroup pass; a device batch that starts 1 .. 17 bytes into its
allocation and ends on its last byte; sample counts that fill one group, spill into a second and into a fourth; and reads in which
a chosen sample decides, alone, with an N in it, and behind decoys that pass level one but are not in S, 64 of them in one wave.
Needs an MI355X: run with -m gpu."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import genestrip_amd as ga
from genestrip_amd import synth
import matchcheck
import prefilter as pf
import prefilter_cases as pc
import test_gpu_prefilter as tgp
from oracle import gs_oracle as orc
from prefilter import make_reads

pytestmark = pytest.mark.gpu

R = 64    # reads per wave round: one per lane
T = 1024  # reads per workgroup pass: GS_PF_READS = GS_PF_BLOCK (256) x GS_PF_ROUNDS (4) of gs_prefilter.hip


@pytest.fixture(scope="module")
def db31():
    return synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)


@pytest.fixture(scope="module")
def st31(db31):
    s = tgp._Store(31, db31.kmers, db31.value_idx, db31.n_values, db31.parent_vi)
    yield s
    s.close()


@pytest.fixture(scope="module")
def S31(db31):
    return pf.lmer_set(db31.kmers, 31)


@pytest.fixture(scope="module")
def mix31(db31):
    return tgp._reads(db31.genomes, 150, 2 * T + R + 1, seed=151)


@pytest.mark.parametrize("n", [R - 1, R, R + 1, T - 1, T, T + 1, 2 * T + R + 1])
def test_batch_sizes(st31, S31, mix31, n):
    seq, bg = mix31
    _, info = tgp._check(st31, seq, 150, n, f"{n} reads", bg=bg)
    assert info["survivors"] == int(pf.passes(S31, seq[:n], 150, 31).sum())


@pytest.mark.parametrize("L", [151, 150])
@pytest.mark.parametrize("o", [1, 2, 3, 15, 17])
def test_alignment(st31, db31, S31, o, L):
    """the batch is a view o bytes into a 16-byte-aligned device allocation of exactly o + n L bytes: the first piece of the first
    round and the last piece of the last are cut, and no byte beside the batch exists behind it"""
    n = T + R + 1
    seq, _ = tgp._reads(db31.genomes, L, n, seed=1000 + 16 * L + o)
    buf = torch.empty(o + n * L, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[o:o + n * L]
    view.copy_(torch.from_numpy(seq.reshape(-1)))
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    want = matchcheck.oracle_batch(st31.odb, seq.reshape(-1), off)
    got = {}
    for mode in (1, 0):
        before = os.environ.pop("GS_PREFILTER", None)
        os.environ["GS_PREFILTER"] = str(mode)
        try:
            m = ga.FastqKMerMatcher(st31.dev, ga.MatchConfig())
        finally:
            os.environ.pop("GS_PREFILTER", None)
            if before is not None:
                os.environ["GS_PREFILTER"] = before
        try:
            cv = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            fl = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
            m.submit_fixed(view, L, n, 0, class_vi=cv, flags=fl)
            info = m.prefilter_info()
            t, d = m.finish()
        finally:
            m.close()
        got[mode] = dict(table=t, dtable=d, class_vi=cv.cpu().numpy(), flags=fl.cpu().numpy())
        matchcheck.check_match(want, got[mode], f"offset {o} L {L} prefilter {mode}")
        if mode == 1:
            assert info["reads"] == n and info["survivors"] == int(pf.passes(S31, seq, L, 31).sum()), info
        else:
            assert info["survivors"] == -1
    assert np.array_equal(got[1]["table"], got[0]["table"])
    assert np.array_equal(got[1]["class_vi"], got[0]["class_vi"]) and np.array_equal(got[1]["flags"], got[0]["flags"])


class _PfParams(C.Structure):  # GsPrefilterParams of genestrip_amd/csrc/gs_params.h
    _fields_ = [("seq", C.c_void_p), ("n_reads", C.c_int64), ("L", C.c_int32), ("k", C.c_int32), ("l1", C.c_void_p), ("l2", C.c_void_p),
                ("list", C.c_void_p), ("count", C.c_void_p), ("class_vi", C.c_void_p), ("flags", C.c_void_p)]


def _bit_table(bits, n_words):
    t = np.zeros(n_words, dtype=np.uint32)
    bits = np.asarray(bits, dtype=np.int64)
    np.bitwise_or.at(t, bits >> 5, (np.uint32(1) << (bits & 31).astype(np.uint32)))
    return torch.from_numpy(t.view(np.int32)).cuda()


def _launch_kernel(S, seq, L, k):
    """gs_launch_prefilter itself on the batch `seq` (n, L) against both levels of S (built here from tests/prefilter.py's set): ->
    (the list up to the count, the whole list, class_vi, flags), the outputs preset to values the kernel does not write"""
    n = len(seq)
    l1 = _bit_table(pc.l1_bits(S), 1 << 19)
    l2 = _bit_table(S, 1 << 25)
    d_seq = torch.from_numpy(np.ascontiguousarray(seq).reshape(-1)).cuda()
    lst = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    cv = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    fl = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    P = _PfParams(d_seq.data_ptr(), n, L, k, l1.data_ptr(), l2.data_ptr(), lst.data_ptr(), count.data_ptr(), cv.data_ptr(), fl.data_ptr())
    torch.cuda.synchronize()
    fn = ga.lib().gs_launch_prefilter
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    assert fn(C.byref(P), None) == 0
    torch.cuda.synchronize()
    c = int(count.item())
    assert 0 <= c <= n
    lst = lst.cpu().numpy()
    return lst[:c], lst, cv.cpu().numpy(), fl.cpu().numpy()


@pytest.mark.parametrize("k,L,m", [(31, 95, 5), (31, 158, 9), (25, 152, 13), (19, 83, 14), (19, 146, 27)])
def test_sample_counts(k, L, m):
    """m samples: sample 0, then groups of eight -- a short group, one full group, and up to four groups.
    The kernel is launched on its own (gs_launch_prefilter) at every (k, L): the list holds exactly the reads tests/prefilter.py
    lets pass, each once, and exactly the rejected reads get -1 / 0.  Through the library the full _check holds where the library
    sends a batch of this length through the prefilter -- from L = 128 on, the FIXED loop of the match kernel -- and m = 5
    (L = 95) and m = 14 (L = 83) lie below that: there prefilter_info() must say so (survivors -1), and forced on, forced off and
    the oracle still agree in every output."""
    assert len(pf.sample_positions(L, k)) == m
    db = synth.SynthDB(k=k, genera=2, species_per_genus=3, genome_len=20000, seed=3)
    S = pf.lmer_set(db.kmers, k)
    n = 1500
    seq = make_reads(db.genomes, L, k, n, seed=100 * k + L)
    ok = pf.passes(S, seq, L, k)
    assert 0 < ok.sum() < n
    got, whole, cv, fl = _launch_kernel(S, seq, L, k)
    assert np.array_equal(np.sort(got), np.flatnonzero(ok)), (len(got), int(ok.sum()))
    assert np.all(whole[len(got):] == -5)
    assert np.all(cv[~ok] == -1) and np.all(fl[~ok] == 0) and np.all(cv[ok] == -7) and np.all(fl[ok] == 0xEE)
    s = tgp._Store(k, db.kmers, db.value_idx, db.n_values, db.parent_vi)
    try:
        if L >= 128:
            _, info = tgp._check(s, seq, L, n, f"k {k} L {L}", bg=np.arange(n) % 4 == 3)
            assert info["survivors"] == int(ok.sum())
        else:
            off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
            o = matchcheck.oracle_batch(s.odb, seq.reshape(-1), off)
            on, info_on = tgp._device(s, 1, [(seq, n, 0)], L)
            offr, _ = tgp._device(s, 0, [(seq, n, 0)], L)
            assert info_on[0]["reads"] == n and info_on[0]["survivors"] == -1, info_on
            matchcheck.check_match(o, on, f"k {k} L {L} prefilter on")
            matchcheck.check_match(o, offr, f"k {k} L {L} prefilter off")
            assert np.array_equal(on["table"], offr["table"])
    finally:
        s.close()


def test_which_sample_decides(st31, db31, S31):
    """every sample index decides a read: alone, with an N in it (rejected), and behind two to four decoys; the decoy reads of a
    wave sit between genome reads, so that its lanes need different numbers of exact-level steps"""
    reads, expect, decider, _ = pc.deciding_sample_reads(S31, 150, 31, seed=9)
    led = reads[2::3]  # the decoy reads, one per sample index
    rng = np.random.default_rng(3)
    wave = np.concatenate([led[rng.integers(0, len(led), 64 - len(led))], led])  # 64 of them ...
    genome, _ = tgp._reads(db31.genomes, 150, 64, seed=77, background="none")
    pad, _ = tgp._reads(db31.genomes, 150, -len(reads) % 64, seed=78, background="none")  # the 64 decoy reads fill one wave round
    mixed = np.empty((128, 150), dtype=np.uint8)  # ... mixed with genome reads over two wave rounds
    mixed[0::2], mixed[1::2] = wave, genome
    seq = np.ascontiguousarray(np.concatenate([reads, pad, wave, mixed]))
    n = len(seq)
    assert (len(reads) + len(pad)) % 64 == 0
    ok = pf.passes(S31, seq, 150, 31)
    assert ok[:len(reads)].tolist() == expect.tolist() and ok[len(reads) + len(pad):len(reads) + len(pad) + 64].all()
    _, info = tgp._check(st31, seq, 150, n, "which sample decides")
    assert info["survivors"] == int(ok.sum())
