"""The split pipeline (gs_route.hip: gs_encode_kernel, gs_encode_route_kernel, gs_route_*_kernel, gs_unroute_kernel,
gs_probe_keys_kernel, and the FROM_NODES reduce) at every k class -- no minimizer gate (16), the first k with one (19), both sides of
the context-key boundary of plain stores (21, 22; partition gates stay minimizer-keyed), 25 and 31 -- and the routing kernels on
synthetic key tensors at their tile edges and owner counts.

The key of every k-mer position is held to tests/planarkey.py, a restatement of the key scheme that does not call the library: all
ranks must agree on the key that crosses the wire, and store files depend on it."""
import numpy as np
import pytest
import torch

import genestrip_amd as ga
import matchcheck
import planarkey as pk
import splitpipe
from genestrip_amd import distributed as gd
from genestrip_amd import synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
KS = (16, 19, 21, 22, 25, 31)
GS_E_INVALID = -1


class Case:
    """store arrays at one k, a batch of about 3 000 reads, the oracle's result, planarkey's key of every k-mer position"""

    def __init__(self, k):
        self.k = k
        self.sdb = sdb = synth.SynthDB(k=k, genera=3, species_per_genus=3, genome_len=10000, seed=11)
        rng = np.random.default_rng(1000 + k)
        g = sdb.genomes

        def piece(n):
            p = int(rng.integers(0, g.shape[1] - n + 1))
            return g[int(rng.integers(0, len(g)))][p:p + n].copy()

        reads = []
        # lengths at the edges of the sub-rounds of 64 and 128 positions and of the first-192-bases prefetch of gs_encode_kernel
        for n in [p + k - 1 for p in (1, 127, 128, 129, 192 - k + 1, 193 - k + 1)] + [k - 1, k, 0, 191, 192, 193]:
            for variant in range(4):
                r = piece(n)
                if variant == 1 and n:
                    r[n - 1] = ord("N")
                if variant == 2 and n:
                    r[0] = ord("n")
                if variant == 3:
                    r[n // 2:] |= 0x20
                reads.append(r)
        for i in range(2400):
            r = piece(150)
            hit = np.flatnonzero(rng.random(150) < 0.01)
            r[hit] = ACGT[rng.integers(0, 4, len(hit))]
            if i % 40 == 0:
                r[int(rng.integers(0, 150))] = ord("N")
            if i % 40 == 1:
                a = int(rng.integers(0, 140))
                r[a:a + 10] |= 0x20
            reads.append(r)
        reads += [piece(int(n)) for n in rng.integers(k, 400, 200)]
        reads += [ACGT[rng.integers(0, 4, int(n))] for n in rng.integers(k, 300, 350)]  # from elsewhere: the gate stops most of their k-mers
        reads = [reads[i] for i in rng.permutation(len(reads))]
        lens = np.array([len(r) for r in reads], dtype=np.uint64)
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        self.seq = np.ascontiguousarray(np.concatenate(reads).astype(np.uint8))
        self.odb = orc.DB(k, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
        self.oracle = matchcheck.oracle_batch(self.odb, self.seq, self.off)
        # every k-mer position of the batch, in read order: the window's key, whether it is valid, whether the oracle holds it
        wk, wv = pk.window_keys_np(self.seq, k)
        off = self.off.astype(np.int64)
        cnt = np.maximum(off[1:] - off[:-1] - (k - 1), 0)
        self.pos_off = np.concatenate([[0], np.cumsum(cnt)])
        at = np.repeat(off[:-1] - self.pos_off[:-1], cnt) + np.arange(self.pos_off[-1])
        self.key, self.valid = wk[at], wv[at]
        canon = pk.kmers_of_planes_np(*pk.unmix_np(self.key), k)
        self.held = np.isin(canon, sdb.kmers) & self.valid
        # validity and "held" as the oracle has them, on a sample and on every window that touches a foreign byte: a window is valid
        # iff the oracle's k-mer routine finds no bad position in it (upper-case ACGT only: for the reference's matcher a lower-case
        # base is as foreign as an N), and np.isin over the oracle's array is the oracle's lookup
        near_bad = np.flatnonzero(~self.valid)
        for i in np.concatenate([rng.choice(len(at), 1500, replace=False), near_bad[::3], near_bad[:-1][np.diff(near_bad) > 1] + 1]):
            w = self.seq[at[i]:at[i] + k].tobytes()
            assert (orc.kmer_straight(w, 0, k)[1] == -1) == bool(self.valid[i])
            if self.valid[i]:
                assert orc.kmer_canonical(w, 0, k) == canon[i]
                assert (self.odb.get(int(canon[i]))[0] >= 0) == bool(self.held[i])
        assert 0.5 < self.held.mean() < 0.95 and 100 < (~self.valid).sum()

    def stores(self, world):
        s = self.sdb
        return [ga.DeviceKMerStore(self.k, s.kmers, s.value_idx, s.n_values, s.parent_vi, n_parts=world, part=p, partition=True)
                for p in range(world)]


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(k):
        if k not in made:
            made[k] = Case(k)
        return made[k]
    return get


def _check_keys(c, keys, what):
    """one key per k-mer position: KEY_INVALID exactly at the windows the oracle calls invalid (a byte outside upper-case ACGT: the
    reference's matcher treats a lower-case base like an N, and the whole-result check below depends on it), elsewhere planarkey's
    key, or KEY_MISS where the oracle does not hold the k-mer (never at k < 19: no gate)"""
    assert keys.shape == c.key.shape, what
    inv = keys == gd.KEY_INVALID
    assert np.array_equal(inv, ~c.valid), (what, np.flatnonzero(inv != ~c.valid)[:8].tolist())
    miss = keys == gd.KEY_MISS
    assert not (miss & c.held).any(), (what, "a stored k-mer stopped at the gate", np.flatnonzero(miss & c.held)[:8].tolist())
    rest = ~inv & ~miss
    bad = np.flatnonzero(rest & (keys != c.key))
    assert bad.size == 0, (what, len(bad), keys[bad[:4]].tolist(), c.key[bad[:4]].tolist())
    if c.k < 19:
        assert not miss.any(), what
    else:
        assert miss.sum() > 10000, what  # the gate is at work: most k-mers of the reads from elsewhere
    return miss


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("k", KS)
def test_encode_and_pipeline(cases, k, world):
    c = cases(k)
    stores = c.stores(world)
    try:
        assert sum(s.info.n_stored for s in stores) == len(c.sdb.kmers)
        for s in stores:
            assert (s.info.mgate_bytes > 0) == (k >= 19) and s.info.n_in_records == 0
        misses = []
        for device_routing in (True, False):
            res = splitpipe.run(stores, k, c.seq, c.off, device_routing)
            what = f"k {k}, world {world}, device routing {device_routing}"
            keys = np.concatenate(res["keys"])
            misses.append(_check_keys(c, keys, what))
            for p, (recv, nodes) in enumerate(res["probed"]):
                assert np.all(pk.owner(recv, world) == p), what
            matchcheck.check_match_parts(c.oracle, res["parts"], what)
        assert np.array_equal(misses[0], misses[1])
        miss = misses[0]
        # encode and routing in one kernel, on the whole batch, by the last rank
        n = len(c.off) - 1
        dev = torch.device("cuda")
        m = ga.FastqKMerMatcher(stores[-1])
        dseq = torch.from_numpy(c.seq).to(dev)
        doff = torch.from_numpy(c.off.astype(np.int64)).to(dev)
        pos_off = gd.position_offsets(doff, k)
        assert np.array_equal(pos_off.cpu().numpy(), c.pos_off)
        nk = int(c.pos_off[-1])
        waves, chunk = m.route_geometry(n)
        cap = ((nk // world) * 2 + (waves + 2) * chunk + chunk - 1) // chunk * chunk
        sk = torch.empty(world * cap, dtype=torch.int64, device=dev)
        si = torch.empty(world * cap, dtype=torch.int32, device=dev)
        nodes = torch.full((nk,), -9, dtype=torch.int32, device=dev)
        counts, over = m.encode_route(dseq, doff, pos_off, n, world, cap, sk, si, nodes)
        m.close()
        assert not over
        routed = c.valid & ~miss
        own = pk.owner(c.key, world)
        for o in range(world):
            rk, ri = sk[o * cap:o * cap + counts[o]].cpu().numpy(), si[o * cap:o * cap + counts[o]].cpu().numpy()
            used = ri != -1
            assert counts[o] % chunk == 0 and np.all(rk[~used] == -1)  # whole chunks, sentinels in the unused slots
            want_i = np.flatnonzero(routed & (own == o))
            order = np.argsort(ri[used], kind="stable")
            assert np.array_equal(ri[used][order], want_i), (k, world, o)
            assert np.array_equal(rk[used][order], c.key[want_i]), (k, world, o)
        got = nodes.cpu().numpy()
        assert np.all(got[~c.valid] == gd.NODE_INVALID) and np.all(got[miss] == gd.NODE_MISS) and np.all(got[routed] == gd.NODE_MISS)
    finally:
        for s in stores:
            s.close()


@pytest.fixture(scope="module")
def handle():
    """a partition store of one entry: the routing calls need a run handle, not a store"""
    kmer = orc.kmer_canonical(b"ACGTTGCAAGGCTTAACCGGTACGATCGATA", 0, 31)
    store = ga.DeviceKMerStore(31, np.array([kmer], dtype=np.int64), np.array([1], dtype=np.int32), 2, np.array([-1, 0], dtype=np.int32),
                               n_parts=1, part=0, partition=True)
    m = ga.FastqKMerMatcher(store)
    yield m
    m.close()
    store.close()


def _synthetic_keys(n, n_parts, mix, rng):
    keys = rng.integers(0, 1 << 62, n, dtype=np.int64)
    if mix == "one-owner":  # the last owner takes every key
        q = rng.integers(0, (1 << 22) // n_parts, n, dtype=np.int64)
        keys = ((q * n_parts + (n_parts - 1)) << pk.OWNER_SHIFT) | (keys & ((1 << pk.OWNER_SHIFT) - 1))
    elif mix == "none":
        keys = np.where(rng.integers(0, 2, n) == 0, gd.KEY_MISS, gd.KEY_INVALID).astype(np.int64)
    else:
        u = rng.random(n)
        keys[u < 0.10] = gd.KEY_MISS
        keys[u < 0.05] = gd.KEY_INVALID
    return keys


@pytest.mark.parametrize("n_parts", [1, 2, 3, 7, 64])
def test_route_and_unroute_on_synthetic_keys(handle, n_parts):
    """gs_route_keys against plan_routing, gs_unroute_nodes (both forms) against scatter_nodes: key counts at the edges of a wave
    (64) and of a workgroup's tile (4096), every owner count class, all keys to one owner, none routed, uniform"""
    m = handle
    dev = torch.device("cuda")
    rng = np.random.default_rng(n_parts)
    for n in (1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 1):
        for mix in ("one-owner", "none", "uniform"):
            what = (n_parts, n, mix)
            hk = _synthetic_keys(n, n_parts, mix, rng)
            keys = torch.from_numpy(hk).to(dev)
            pidx, psend, pcounts = gd.plan_routing(keys, n_parts)
            pcounts = pcounts.cpu().numpy()
            assert pcounts.sum() == (hk >= 0).sum()
            if mix == "one-owner":
                assert pcounts[-1] == n
            send = torch.full((n + 1,), 777, dtype=torch.int64, device=dev)
            idx = torch.full((n + 1,), 777, dtype=torch.int32, device=dev)
            early = torch.full((n + 1,), -9, dtype=torch.int32, device=dev)
            counts = np.array(m.route_keys(keys, n, n_parts, send, idx, early), dtype=np.int64)
            assert np.array_equal(counts, pcounts), what
            total = int(counts.sum())
            assert int(send[total:].eq(777).sum()) == n + 1 - total and int(idx[total:].eq(777).sum()) == n + 1 - total, what
            gs, gi, ps, pi = send[:total].cpu().numpy(), idx[:total].cpu().numpy(), psend.cpu().numpy(), pidx.cpu().numpy()
            start = 0
            for o in range(n_parts):  # the same positions with the same keys in every owner's group, in any order
                a, b = slice(start, start + counts[o]), np.argsort(gi[start:start + counts[o]], kind="stable")
                assert np.array_equal(gi[a][b], np.sort(pi[a])) and np.array_equal(gs[a][b], hk[gi[a][b]]), what
                assert np.array_equal(np.sort(gs[a]), np.sort(ps[a])), what
                start += counts[o]
            he = early.cpu().numpy()
            want_early = np.where(hk >= 0, -9, np.where(hk == gd.KEY_MISS, gd.NODE_MISS, gd.NODE_INVALID))
            assert np.array_equal(he[:n], want_early) and he[n] == -9, what
            # the second form of gs_route_keys: no nodes
            send2 = torch.empty(n, dtype=torch.int64, device=dev)
            idx2 = torch.empty(n, dtype=torch.int32, device=dev)
            assert m.route_keys(keys, n, n_parts, send2, idx2, None) == counts.tolist(), what
            # answers come back in the order the keys left: any function of the key will do
            back = (send[:total] % 1009).to(torch.int32)
            want = gd.scatter_nodes((psend % 1009).to(torch.int32), pidx, n, keys).cpu().numpy()
            m.unroute_nodes(None, idx, back, total, early, n)  # the unrouted positions are in `early` already
            full = torch.full((n + 1,), -9, dtype=torch.int32, device=dev)
            m.unroute_nodes(keys, idx, back, total, full, n)
            m.sync()
            assert np.array_equal(early.cpu().numpy()[:n], want) and np.array_equal(full.cpu().numpy()[:n], want), what
            assert int(full[n].item()) == -9 and int(early[n].item()) == -9, what


@pytest.mark.parametrize("n_parts", [0, 65])
def test_owner_counts_outside_1_to_64_are_refused(handle, n_parts):
    m = handle
    dev = torch.device("cuda")
    keys = torch.arange(100, dtype=torch.int64, device=dev) << pk.OWNER_SHIFT
    send = torch.empty(100, dtype=torch.int64, device=dev)
    idx = torch.empty(100, dtype=torch.int32, device=dev)
    with pytest.raises(ga.GsError) as e:
        m.route_keys(keys, 100, n_parts, send, idx, None)
    assert e.value.code == GS_E_INVALID
    seq, off = orc.pack_reads([b"ACGT" * 20, b"TTGACC" * 10])
    dseq = torch.from_numpy(seq).to(dev)
    doff = torch.from_numpy(off.astype(np.int64)).to(dev)
    pos_off = gd.position_offsets(doff, 31)
    cap = gd.ROUTE_CHUNK
    sk = torch.empty(max(n_parts, 1) * cap, dtype=torch.int64, device=dev)
    si = torch.empty(max(n_parts, 1) * cap, dtype=torch.int32, device=dev)
    nodes = torch.empty(int(pos_off[-1].item()), dtype=torch.int32, device=dev)
    with pytest.raises(ga.GsError) as e:
        m.encode_route(dseq, doff, pos_off, 2, n_parts, cap, sk, si, nodes)
    assert e.value.code == GS_E_INVALID
