"""Every statistics sink of the match path times every kernel family, each cell held to the whole-output checker
(tests/matchcheck.py: integer table, class, flags, max hit counts, every double-table cell).

The statistics tiers (gs_params.h, gs_api.cpp gs_match_begin): counters in LDS up to GS_NV_LDS values; above, global
counters spread over stat copies (halved while copies * n_values * 96 B > 64 MiB), reads of one tax id deferred into GsStatRec
records that gs_stat_reduce_kernel adds up in passes of GS_REDUCE_VALUES values (gs_stat_vi_kernel first when there is more
than one pass) up to GS_STAT_REC_MAX_VALUES; the taxonomy leaves LDS above GS_NV_TREE_LDS.  The kernel families are chosen
by k-mer positions (read length - k + 1): up to 128 gs_match_kernel, 129 .. 192 / 193 .. 256 the wide kernels (NS = 3 / 4),
above the long-read kernel, from GS_HUGE_MIN the huge-read kernels; submit_fixed of one length above 128 positions goes
straight to the wide or long kernel (no gs_stat_reduce).  Layouts: plain, a 3-stripe striped store, a 2-rank DB-partitioned
reduce (FROM_NODES kernels, emulated in-process as tests/test_gpu_partitioned.py does).

A cell is named "<n_values>/<family>/k<k>/p<max_paths>/<layout>[/ctx][/nouniq][/recs0][/copies<c>][/maxk<m>]".  KERNELS names
for every kernel instantiation of gs_launch_match, gs_launch_match_long, gs_launch_match_wide and gs_launch_match_huge the
cell that reaches it (tests/test_stats_tiers_cpu.py holds the table to the launch code); each cell asserts the preconditions
that select its kernels.  GS_FORCE_GLOBAL_STATS is not used: gs_kernels.hip caches it in a static while gs_api.cpp reads it
on every run, so a test that set it would make results depend on test order.  Needs an MI355X: run with -m gpu."""
import json
import os
import re
import zlib

import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
from oracle import gs_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genestrip_amd", "csrc")

# instantiation (all template arguments, defaults filled in) -> (launch function, cell that reaches it)
KERNELS = {
    # gs_launch_match: <LDS_STATS, FROM_NODES, KC, WIDE, STRIPED, CTX>
    "gs_match_kernel<true, false, 31, false, false, 0>": ("gs_launch_match", "128/short/k31/p10/plain"),
    "gs_match_kernel<false, false, 31, false, false, 0>": ("gs_launch_match", "641/short/k31/p10/plain"),
    "gs_match_kernel<true, false, 31, false, false, 1>": ("gs_launch_match", "128/short/k31/p10/plain/ctx/maxk3"),
    "gs_match_kernel<false, false, 31, false, false, 1>": ("gs_launch_match", "2049/short/k31/p10/plain/ctx"),
    "gs_match_kernel<true, false, 0, false, false, 0>": ("gs_launch_match", "128/short/k25/p10/plain/nouniq"),
    "gs_match_kernel<false, false, 0, false, false, 0>": ("gs_launch_match", "1281/short/k25/p10/plain/maxk3"),
    "gs_match_kernel<true, false, 0, false, false, 1>": ("gs_launch_match", "128/short/k25/p10/plain/ctx"),
    "gs_match_kernel<false, false, 0, false, false, 1>": ("gs_launch_match", "10241/short/k25/p10/plain/ctx"),
    "gs_match_kernel<true, false, 0, true, false, 2>": ("gs_launch_match", "128/short/k31/p128/plain"),
    "gs_match_kernel<false, false, 0, true, false, 2>": ("gs_launch_match", "640/short/k25/p128/plain/recs0"),
    "gs_match_kernel<true, false, 31, false, true, 0>": ("gs_launch_match", "128/short/k31/p10/striped"),
    "gs_match_kernel<false, false, 31, false, true, 0>": ("gs_launch_match", "2048/short/k31/p10/striped"),
    "gs_match_kernel<true, false, 31, false, true, 1>": ("gs_launch_match", "128/short/k31/p10/striped/ctx"),
    "gs_match_kernel<false, false, 31, false, true, 1>": ("gs_launch_match", "129/short/k31/p10/striped/ctx"),
    "gs_match_kernel<true, false, 0, false, true, 0>": ("gs_launch_match", "128/short/k25/p10/striped/copies1"),
    "gs_match_kernel<false, false, 0, false, true, 0>": ("gs_launch_match", "10240/short/k25/p10/striped"),
    "gs_match_kernel<true, false, 0, false, true, 1>": ("gs_launch_match", "128/short/k25/p10/striped/ctx"),
    "gs_match_kernel<false, false, 0, false, true, 1>": ("gs_launch_match", "50000/short/k25/p10/striped/ctx"),
    "gs_match_kernel<true, false, 0, true, true, 2>": ("gs_launch_match", "128/short/k31/p128/striped"),
    "gs_match_kernel<false, false, 0, true, true, 2>": ("gs_launch_match", "1281/short/k25/p128/striped/copies64"),
    "gs_match_kernel<true, true, 0, false, false, 0>": ("gs_launch_match", "128/short/k31/p10/part"),
    "gs_match_kernel<false, true, 0, false, false, 0>": ("gs_launch_match", "641/short/k31/p10/part"),
    "gs_match_kernel<true, true, 0, true, false, 0>": ("gs_launch_match", "128/short/k25/p128/part"),
    "gs_match_kernel<false, true, 0, true, false, 0>": ("gs_launch_match", "2049/short/k31/p128/part"),
    # gs_launch_match_long: <LDS_STATS, FROM_NODES, WIDE, STRIPED, KC>
    "gs_match_long_kernel<true, false, true, true, 0>": ("gs_launch_match_long", "128/long300/k31/p128/striped"),
    "gs_match_long_kernel<false, false, true, true, 0>": ("gs_launch_match_long", "10241/long300/k25/p128/striped"),
    "gs_match_long_kernel<true, false, false, true, 0>": ("gs_launch_match_long", "128/long300/k31/p10/striped"),
    "gs_match_long_kernel<false, false, false, true, 0>": ("gs_launch_match_long", "641/long1400/k31/p10/striped"),
    "gs_match_long_kernel<true, false, true, false, 0>": ("gs_launch_match_long", "128/long300/k31/p128/plain"),
    "gs_match_long_kernel<false, false, true, false, 0>": ("gs_launch_match_long", "129/long1400/k25/p128/plain"),
    "gs_match_long_kernel<true, true, true, false, 0>": ("gs_launch_match_long", "128/long300/k31/p128/part"),
    "gs_match_long_kernel<false, true, true, false, 0>": ("gs_launch_match_long", "1281/long300/k25/p128/part"),
    "gs_match_long_kernel<true, false, false, false, 31>": ("gs_launch_match_long", "128/long300/k31/p10/plain/maxk3"),
    "gs_match_long_kernel<false, false, false, false, 31>": ("gs_launch_match_long", "2048/long1400/k31/p10/plain"),
    "gs_match_long_kernel<true, false, false, false, 0>": ("gs_launch_match_long", "128/long300/k25/p10/plain"),
    "gs_match_long_kernel<false, false, false, false, 0>": ("gs_launch_match_long", "640/long300/k25/p10/plain/maxk3"),
    "gs_match_long_kernel<true, true, false, false, 0>": ("gs_launch_match_long", "128/long1400/k31/p10/part"),
    "gs_match_long_kernel<false, true, false, false, 0>": ("gs_launch_match_long", "10240/long300/k31/p10/part"),
    # gs_launch_match_wide: <LDS_STATS, NS, KC>
    "gs_match_wide_kernel<false, 3, 0>": ("gs_launch_match_wide", "2049/wide3/k25/p10/plain"),
    "gs_match_wide_kernel<false, 3, 31>": ("gs_launch_match_wide", "641/wide3/k31/p10/plain/maxk3"),
    "gs_match_wide_kernel<false, 4, 0>": ("gs_launch_match_wide", "129/wide4/k25/p10/plain"),
    "gs_match_wide_kernel<false, 4, 31>": ("gs_launch_match_wide", "10241/fixed250/k31/p10/plain"),
    "gs_match_wide_kernel<true, 3, 0>": ("gs_launch_match_wide", "128/wide3/k25/p10/plain"),
    "gs_match_wide_kernel<true, 3, 31>": ("gs_launch_match_wide", "128/wide3/k31/p10/plain"),
    "gs_match_wide_kernel<true, 4, 0>": ("gs_launch_match_wide", "128/fixed250/k25/p10/plain"),
    "gs_match_wide_kernel<true, 4, 31>": ("gs_launch_match_wide", "128/wide4/k31/p10/plain/maxk3"),
    # gs_launch_match_huge: <LDS_STATS, STRIPED, KC> and the finish kernel <LDS_STATS>
    "gs_match_huge_kernel<true, true, 0>": ("gs_launch_match_huge", "128/huge/k31/p10/striped"),
    "gs_match_huge_kernel<true, false, 31>": ("gs_launch_match_huge", "128/huge/k31/p10/plain"),
    "gs_match_huge_kernel<true, false, 0>": ("gs_launch_match_huge", "128/huge/k25/p128/plain"),
    "gs_match_huge_finish_kernel<true>": ("gs_launch_match_huge", "128/huge/k31/p10/plain"),
    "gs_match_huge_kernel<false, true, 0>": ("gs_launch_match_huge", "2048/huge/k25/p10/striped"),
    "gs_match_huge_kernel<false, false, 31>": ("gs_launch_match_huge", "400000/huge/k31/p10/plain"),
    "gs_match_huge_kernel<false, false, 0>": ("gs_launch_match_huge", "641/huge/k25/p10/plain"),
    "gs_match_huge_finish_kernel<false>": ("gs_launch_match_huge", "400000/huge/k31/p10/plain/maxk3"),
}

TIERS = [128, 129, 640, 641, 1281, 2048, 2049, 10240, 10241, 50000, 400000]
FAMILIES = ["short", "wide3", "wide4", "long300", "long1400", "huge", "mixed", "fixed250"]
READ_LEN = {"short": 150, "wide3": 200, "wide4": 250, "long300": 300, "long1400": 1400, "huge": 1400, "fixed250": 250}
MIXED_LENS = (31, 40, 99, 150, 151, 180, 200, 222, 250, 286, 300, 700, 1400)
HUGE_MIN = 300  # GS_HUGE_MIN of the huge cells (k-mer positions)
STATS = ["", "recs0", "copies1", "copies64"]
LAYOUTS = ["plain", "striped", "part"]


def sweep_cells():
    """every tier times every family; k, max_paths, count_unique, the statistics knobs and the layout rotate over the cells so
    that every pair of their values comes up (tests/test_stats_tiers_cpu.py checks that)"""
    out = []
    for f, fam in enumerate(FAMILIES):
        for t, nv in enumerate(TIERS):
            i = f * len(TIERS) + t
            layout = LAYOUTS[i % 3]
            if layout == "part" and fam in ("huge", "fixed250"):  # (no huge kernels and no fixed-length batches from nodes)
                layout = "striped"
            tags = [str(nv), fam, "k%d" % (31, 25)[(i // 3) % 2], "p%d" % (10, 128)[(i // 6 + i) % 2], layout]
            if (i // 2) % 2:
                tags.append("nouniq")
            if STATS[(i // 4 + i) % 4]:
                tags.append(STATS[(i // 4 + i) % 4])
            if layout == "plain" and (i // 9) % 2 == 0 and (i // 2) % 2 == 0:  # (max hit counts need count_unique)
                tags.append("maxk3")
            out.append("/".join(tags))
    return out


def parse_cell(cell):
    tags = cell.split("/")
    c = dict(nv=int(tags[0]), family=tags[1], k=int(tags[2][1:]), paths=int(tags[3][1:]), layout=tags[4], ctx=False,
             unique=True, recs=True, copies=None, maxk=0)
    for t in tags[5:]:
        if t == "ctx":
            c["ctx"] = True
        elif t == "nouniq":
            c["unique"] = False
        elif t == "recs0":
            c["recs"] = False
        elif t.startswith("copies"):
            c["copies"] = int(t[6:])
        elif t.startswith("maxk"):
            c["maxk"] = int(t[4:])
        else:
            raise ValueError(cell)
    assert c["family"] in FAMILIES and c["layout"] in LAYOUTS and c["k"] in (25, 31) and c["paths"] in (10, 128), cell
    assert not (c["layout"] == "part" and (c["family"] in ("huge", "fixed250") or c["maxk"])), cell
    assert not (c["layout"] == "striped" and c["maxk"]) and not (c["maxk"] and not c["unique"]), cell
    return c


def cells():
    return sorted(set(sweep_cells()) | {v[1] for v in KERNELS.values()}, key=lambda s: (int(s.split("/")[0]), s))


def defines():
    """the tier limits of the launch code: #defines of gs_params.h and GS_REDUCE_VALUES of gs_kernels.hip"""
    out = {}
    for name in ("gs_params.h", "gs_kernels.hip"):
        for m in re.finditer(r"^#define\s+(GS_\w+)\s+([^\n/]+)", open(os.path.join(CSRC, name)).read(), re.M):
            v = m.group(2).strip()
            if re.fullmatch(r"[\d\s()<]+", v):  # (numbers and shifts only)
                out.setdefault(m.group(1), int(eval(v)))
    return out


# ------------------------------------------------------------------ the store: boundary rows, a deep tree
GENERA, SPECIES, STRAINS, SEGMENTS, SEG_LEN = 2, 2, 2, 5, 1500


def target_rows(nv, d):
    """rows next to every tier boundary, the first and last row of every reduce pass, and n_values - 1"""
    rows = {127, 128, 639, 640, 641, 1279, 1280, 2047, 2048, 10239, 10240, nv - 1}
    rv = d["GS_REDUCE_VALUES"]
    for p in range(min((nv + rv - 1) // rv, d["GS_STAT_REC_MAX_VALUES"] // rv)):
        rows |= {p * rv, p * rv + rv - 1}
    return sorted((r for r in rows if 0 < r < nv), reverse=True)


class Material:
    """genomes of 2 genera x 2 species x 2 strains, each strain cut into 5 leaves; shared blocks put k-mers on the species and
    genus nodes and k-mers across leaf seams on the strain nodes (DbBuild: k-mer -> LCA of the leaves that hold it)"""

    def __init__(self, seed=31):
        rng = np.random.default_rng(seed)
        L = SEGMENTS * SEG_LEN
        acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
        gcore = [rng.choice(acgt, L) for _ in range(GENERA)]
        score = [rng.choice(acgt, L) for _ in range(GENERA * SPECIES)]
        genomes = []
        for g in range(GENERA):
            for s in range(SPECIES):
                for t in range(STRAINS):
                    gen = rng.choice(acgt, L)
                    for b in range(L // 250):
                        blk = slice(b * 250, (b + 1) * 250)
                        if b % 7 == 3:
                            gen[blk] = gcore[g][blk]
                        elif b % 5 == 1:
                            gen[blk] = score[g * SPECIES + s][blk]
                    genomes.append(gen)
        self.genomes = np.stack(genomes)
        self.genus_of = np.repeat(np.arange(GENERA), SPECIES * STRAINS)


class Store:
    def __init__(self, mat, nv, k, d):
        rng = np.random.default_rng(nv * 100 + k)
        n_strain = GENERA * SPECIES * STRAINS
        # nodes: 0 root, genera, species, strains (internal), then the leaves
        kind_parent = [-1] + [0] * GENERA + [1 + g for g in range(GENERA) for _ in range(SPECIES)]
        kind_parent += [1 + GENERA + s for s in range(GENERA * SPECIES) for _ in range(STRAINS)]
        n_internal = len(kind_parent)
        kind_parent += [n_internal - n_strain + i for i in range(n_strain) for _ in range(SEGMENTS)]
        n_nodes = len(kind_parent)
        assert n_nodes <= nv
        # rows: the root in row 0; over the boundary rows (highest first) internal nodes and leaves alternate; the rest at random
        row = np.full(n_nodes, -1, dtype=np.int64)
        row[0] = 0
        internal, leaves = list(range(n_internal - 1, 0, -1)), list(range(n_internal, n_nodes))
        for j, r in enumerate(target_rows(nv, d)):
            pool = internal if (j % 2 == 0 and internal) or not leaves else leaves
            if pool:
                row[pool.pop(0)] = r
        free = np.setdiff1d(np.arange(1, nv), row[row >= 0])
        rest = np.flatnonzero(row < 0)
        row[rest] = rng.choice(free, len(rest), replace=False)
        parent = np.full(nv, -1, dtype=np.int32)
        used = np.zeros(nv, dtype=bool)
        used[row] = True
        for v in range(1, n_nodes):
            parent[row[v]] = row[kind_parent[v]]
        # the rows without a node: leaves without k-mers under random internal nodes
        spare = np.flatnonzero(~used)
        parent[spare] = row[rng.integers(0, n_internal, len(spare))]
        self.nv, self.k, self.parent, self.row = nv, k, parent, row
        self.leaf_row = row[n_internal:].reshape(n_strain, SEGMENTS)
        seqs, nodes = [], []
        for i in range(n_strain):
            for j in range(SEGMENTS):
                # (neighbouring leaves overlap by 2 (k - 1) bases: the k-mers across a seam go to the strain node)
                seqs.append(mat.genomes[i, max(0, j * SEG_LEN - k + 1):min((j + 1) * SEG_LEN + k - 1, SEGMENTS * SEG_LEN)])
                nodes.append(self.leaf_row[i, j])
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        seq = np.concatenate(seqs)
        b = orc.DbBuild(k, nv, parent)
        b.fill(seq, off, np.array(nodes, dtype=np.int32))
        b.optimize()
        b.update(seq, off, np.array(nodes, dtype=np.int32))
        self.kmers, self.vidx = b.fetch()
        b.close()
        self.odb = orc.DB(k, self.kmers, self.vidx, nv, parent)
        self.dev = {}

    def device(self, layout, ctx, monkeypatch):
        key = (layout, ctx)
        if key not in self.dev:
            with monkeypatch.context() as mp:
                if ctx:
                    mp.setenv("GS_GATE_CTX_MIN_DISTINCT", "1")  # the context-keyed gate of big stores, on this small one
                a = (self.k, self.kmers, self.vidx, self.nv, self.parent)
                if layout == "plain":
                    self.dev[key] = [ga.DeviceKMerStore(*a)]
                elif layout == "striped":
                    self.dev[key] = ga.DeviceKMerStore.striped(*a, devices=(0, 0, 0))
                else:
                    self.dev[key] = [ga.DeviceKMerStore(*a, n_parts=2, part=p, partition=True) for p in range(2)]
        return self.dev[key]

    def close(self):
        for ss in self.dev.values():
            for s in ss:
                s.close()
        self.dev.clear()
        self.odb.close()


_MAT = []
_STORES = {}
WORST = {}  # n_values -> largest dtable ratio


@pytest.fixture(scope="module")
def env():
    yield dict(d=defines())
    for s in _STORES.values():
        s.close()
    _STORES.clear()
    print("\nSTATS TIERS worst dtable ratio per tier: " + json.dumps(WORST))


def _store(nv, k, d):
    if not _MAT:
        _MAT.append(Material())
    if (nv, k) not in _STORES:
        _STORES[(nv, k)] = Store(_MAT[0], nv, k, d)
    return _STORES[(nv, k)]


# ------------------------------------------------------------------ reads
_COMP = np.zeros(256, dtype=np.uint8)
_COMP[list(b"ACGTN")] = list(b"TGCAN")


def _read(mat, rng, L, chimeric):
    G, n = mat.genomes, mat.genomes.shape[1]
    if chimeric:  # two genomes of different genera: several tax ids, the atomic route
        a = int(rng.integers(0, len(G)))
        b = int(rng.choice(np.flatnonzero(mat.genus_of != mat.genus_of[a])))
        h = L // 2
        pa, pb = int(rng.integers(0, n - h)), int(rng.integers(0, n - (L - h)))
        r = np.concatenate([G[a, pa:pa + h], G[b, pb:pb + L - h]])
    else:  # one genome: mostly inside one leaf, one tax id, the deferred record route
        a = int(rng.integers(0, len(G)))
        j = int(rng.integers(0, SEGMENTS))
        lo = min(j * SEG_LEN, n - L) if L <= SEG_LEN else int(rng.integers(0, n - L + 1))
        hi = max(lo, min((j + 1) * SEG_LEN, n) - L) if L <= SEG_LEN else lo
        p = int(rng.integers(lo, hi + 1))
        r = G[a, p:p + L].copy()
    if rng.random() < 0.5:
        r = _COMP[r[::-1]]
    if rng.random() < 0.03:
        r = r.copy()
        r[int(rng.integers(0, L))] = ord("N")
    return r


def reads(mat, family, n, seed):
    """(seq, offsets): n reads of the family's length (mixed: lengths on every queue), a fifth of them chimeric"""
    rng = np.random.default_rng(seed)
    lens = (rng.choice(MIXED_LENS, n) if family == "mixed" else np.full(n, READ_LEN[family])).astype(np.int64)
    rs = [_read(mat, rng, int(L), rng.random() < 0.2) for L in lens]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return np.concatenate(rs).astype(np.uint8), off


def batch_sizes(family):
    """three batches: two into one run, one after reset(); odd sizes leave every wave's last 64-record chunk partly used"""
    base = {"short": 3000, "wide3": 2400, "wide4": 2000, "long300": 1600, "long1400": 300, "huge": 300, "mixed": 2000,
            "fixed250": 2000}[family]
    return (base + 37) | 1, (base // 2 + 61) | 1, (base // 3 + 5) | 1


# ------------------------------------------------------------------ one run of a cell
def _cfg(c):
    return dict(count_unique=c["unique"], max_paths=c["paths"], max_kmer_res_counts=c["maxk"],
                threshold=2 if c["paths"] == 128 else 1)


def _oracle(st, batches, c):
    run = orc.MatchRun(st.odb, **_cfg(c))
    cvs, fls, terms = [], [], []
    for seq, off, first in batches:
        cv, fl, te = run.submit_terms(seq, off, first, threads=8)
        cvs.append(cv)
        fls.append(fl)
        terms.append(te)
    t, d = run.finish()
    o = dict(table=t, dtable=d, class_vi=np.concatenate(cvs), flags=np.concatenate(fls), terms=np.concatenate(terms))
    if c["maxk"]:
        o["max_counts"] = run.max_counts()
    run.close()
    return o


def _submit(m, c, seq, off, first):
    if c["family"] == "fixed250":
        n = len(off) - 1
        cv, fl = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        m.submit_fixed(seq, READ_LEN["fixed250"], n, first, class_vi=cv, flags=fl)
        m.sync()
        return cv, fl
    return m.match_reads(seq, off, first)


def _part_submit(ms, k, seq, off, first):
    """one batch through the split pipeline over two partition ranks on this device: encode, route, probe on the owner, route
    back, reduce on the home rank; the reads are split in two shards.  Returns the per-rank (class, flags)"""
    import torch

    from genestrip_amd import distributed as gd
    dev = torch.device("cuda")
    world = len(ms)
    n = len(off) - 1
    cuts = [0, n // 2 + 3, n]
    shards, plans = [], []
    for r in range(world):
        lo, hi = cuts[r], cuts[r + 1]
        dseq = torch.from_numpy(seq[int(off[lo]):int(off[hi])].copy()).to(dev)
        doff = torch.from_numpy((off[lo:hi + 1] - off[lo]).astype(np.int64)).to(dev)
        pos_off = gd.position_offsets(doff, k)
        nk = int(pos_off[-1].item())
        keys = torch.empty(max(nk, 1), dtype=torch.int64, device=dev)
        ms[r].encode(dseq, doff, pos_off, keys, hi - lo)
        ms[r].sync()
        idx, send, counts = gd.plan_routing(keys[:nk], world)
        shards.append((dseq, doff, pos_off, nk, keys, hi - lo, lo))
        plans.append((idx, send, np.concatenate([[0], np.cumsum(counts.cpu().numpy())])))
    back = [[None] * world for _ in range(world)]
    for j in range(world):
        recv = torch.cat([plans[i][1][int(plans[i][2][j]):int(plans[i][2][j + 1])] for i in range(world)])
        nodes = torch.empty(max(recv.numel(), 1), dtype=torch.int32, device=dev)
        ms[j].probe_keys(recv, nodes, recv.numel())
        ms[j].sync()
        o = 0
        for i in range(world):
            cnt = int(plans[i][2][j + 1] - plans[i][2][j])
            back[i][j] = nodes[o:o + cnt]
            o += cnt
    out = []
    for r, (dseq, doff, pos_off, nk, keys, nr, lo) in enumerate(shards):
        nodes = gd.scatter_nodes(torch.cat(back[r]), plans[r][0], max(nk, 1), keys)
        cv = torch.full((max(nr, 1),), -1, dtype=torch.int32, device=dev)
        fl = torch.zeros(max(nr, 1), dtype=torch.uint8, device=dev)
        ms[r].reduce(dseq, doff, pos_off, nodes, nr, first_read_no=first + lo, class_vi=cv, flags=fl)
        ms[r].sync()
        out.append((cv[:nr].cpu().numpy(), fl[:nr].cpu().numpy()))
    return out


def _preconditions(c, st, stores, batches, d):
    nv, k = c["nv"], c["k"]
    pos = np.concatenate([np.diff(off.astype(np.int64)) for _, off, _ in batches]) - k + 1
    fam = c["family"]
    if fam == "short":
        assert pos.max() <= 128
    elif fam in ("wide3", "wide4", "fixed250"):
        lo, hi = (129, 192) if fam == "wide3" else (193, 256)
        assert pos.min() >= lo and pos.max() <= hi
    elif fam in ("long300", "long1400"):
        assert pos.min() > 256 and pos.max() < d["GS_HUGE_MIN"]
    elif fam == "huge":
        assert pos.min() >= HUGE_MIN
    else:  # every queue: gs_match_kernel's own reads, both wide kernels' and the long-read kernel's
        for lo, hi in ((1, 128), (129, 192), (193, 256), (257, d["GS_HUGE_MIN"] - 1)):
            assert ((pos >= lo) & (pos <= hi)).sum() > 50, (lo, hi)
    info = [s.info for s in stores]
    assert all(i.n_values == nv and i.k == k for i in info)
    if c["layout"] == "part":  # a partition keeps every key in its table (gs_db_create_part)
        assert all(i.rec_bytes == 0 for i in info)
    else:  # k >= GS_MIN_K: the record layout (gs_process_read's REC route)
        assert info[0].rec_bytes > 0 and info[0].n_in_records > 0
    if c["layout"] == "striped":
        assert [i.n_stripes for i in info] == [3, 3, 3] and [i.stripe for i in info] == [0, 1, 2]
    else:
        assert info[0].n_stripes <= 1
    # the tier: which sinks gs_match_begin picks for this store
    lds = nv <= d["GS_NV_LDS"]
    assert lds == (c["nv"] == 128)
    recs = not lds and nv <= d["GS_STAT_REC_MAX_VALUES"] and c["recs"]
    passes = -(-nv // d["GS_REDUCE_VALUES"]) if recs else 0
    copies = c["copies"] or 16
    while not lds and copies > 1 and copies * nv * 96 > (64 << 20):  # (gs_match_begin; test_stats_tiers_cpu holds the numbers to it)
        copies //= 2
    if not lds and c["copies"] is None:  # the tiers of the copy halving: 16 copies, fewer (50 000 values: 8), one (400 000)
        assert copies == {50000: 8, 400000: 1}.get(nv, 16), (nv, copies)
    # ragged batch ends: an odd batch size cannot fill every wave's last 64-record chunk, whatever the grid
    assert all(len(off) % 2 == 0 for _, off, _ in batches)
    return dict(lds=lds, tree_lds=nv <= d["GS_NV_TREE_LDS"], recs=recs, reduce_passes=passes, copies=copies)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", cells())
def test_stats_tier_cell(cell, env, monkeypatch):
    c = parse_cell(cell)
    d = env["d"]
    if c["recs"] is False:
        monkeypatch.setenv("GS_STAT_RECS", "0")
    if c["copies"]:
        monkeypatch.setenv("GS_STAT_COPIES", str(c["copies"]))
    if c["family"] == "huge":
        monkeypatch.setenv("GS_HUGE_MIN", str(HUGE_MIN))  # (gs_match_begin reads it on every run)
    st = _store(c["nv"], c["k"], d)
    stores = st.device(c["layout"], c["ctx"], monkeypatch)
    mat = _MAT[0]
    seed = zlib.crc32(cell.encode())
    sizes = batch_sizes(c["family"])
    batches, first = [], 5000
    for j, n in enumerate(sizes):
        seq, off = reads(mat, c["family"], n, seed + j)
        batches.append((seq, off, first))
        first += n
    tier = _preconditions(c, st, stores, batches, d)
    # the boundary rows hold k-mers: every reduce pass gets counts in its first and last row
    targets = set(target_rows(c["nv"], d))
    assert targets <= set(st.row.tolist())
    assert targets <= set(np.unique(st.vidx).tolist())
    cfg = ga.MatchConfig(**_cfg(c))
    ms = []
    try:
        worst = _run_cell(c, cell, st, stores, batches, cfg, tier, ms)
    finally:
        for m in ms:
            m.close()
    WORST[c["nv"]] = max(WORST.get(c["nv"], 0.0), worst)


def _run_cell(c, cell, st, stores, batches, cfg, tier, ms):
    """the cell's batches through the device and the oracle; ms collects the runs (closed by the caller)"""
    worst = 0.0
    # two batches into one run, then reset() and the third: counters and seen bits must start from zero again
    for what, part in (("run", batches[:2]), ("after reset", batches[2:])):
        o = _oracle(st, part, c)
        if what == "run":
            assert int((o["class_vi"] >= 0).sum()) > len(o["class_vi"]) // 4, cell
            counted = np.flatnonzero(o["table"][:, orc.C_READS] > 0)
            assert counted.size >= 3, cell
        if c["layout"] == "part":
            if what == "run":
                ms += [ga.FastqKMerMatcher(s, cfg) for s in stores]
            else:
                for m in ms:
                    m.reset()
            outs = [[], []]
            for seq, off, f0 in part:
                for r, (cv, fl) in enumerate(_part_submit(ms, c["k"], seq, off, f0)):
                    outs[r].append((cv, fl))
            res = []
            for r, m in enumerate(ms):
                t, dt = m.finish()
                res.append(dict(table=t, dtable=dt))
            # per-read outputs in read order: each batch's shard of rank 0, then rank 1
            cv = np.concatenate([np.concatenate([outs[0][b][0], outs[1][b][0]]) for b in range(len(part))])
            fl = np.concatenate([np.concatenate([outs[0][b][1], outs[1][b][1]]) for b in range(len(part))])
            g = dict(table=matchcheck.merge_tables([x["table"] for x in res]),
                     dtable=matchcheck.sum_dtables([x["dtable"] for x in res]), class_vi=cv, flags=fl)
        else:
            if what == "run":
                ms.append(ga.FastqKMerMatcher(stores[-1], cfg))
            m = ms[0]
            if what != "run":
                m.reset()
            cvs, fls = [], []
            for seq, off, f0 in part:
                cv, fl = _submit(m, c, seq, off, f0)
                cvs.append(cv)
                fls.append(fl)
            t, dt = m.finish()
            g = dict(table=t, dtable=dt, class_vi=np.concatenate(cvs), flags=np.concatenate(fls))
            if c["maxk"]:
                g["max_counts"] = m.max_counts()
        worst = max(worst, matchcheck.check_match(o, g, f"{cell} {what} {tier}"))
    return worst
