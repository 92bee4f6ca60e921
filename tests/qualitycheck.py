"""CPU reference of the dbquality goal (ft/.../finertree/goals/DBQualityCountsGoal.java handleStore :250-289, doMakeThis :137-173,
DBQualityCSVGoal.makeFile) at a Bloom filter fpp of 0, from the unchanged oracle and numpy alone: nothing here calls the
library under test.

  reference_counts   per leaf: the oracle's DbBuild filled with that leaf's regions only gives the distinct canonical k-mers of
                     the leaf under the reference's window / step / DUST rules; np.searchsorted into the store's sorted k-mer
                     array gives the stored value, a parent walk the ancestor test, np.bincount of the store's values the path sums
  quality_csv        the rank aggregation and the CSV in plain Python, doubles as format(x, ".8f")
"""
import numpy as np

from oracle import gs_oracle as orc

AGG_RANKS = ("cellular root", "acellular root", "species", "genus")
HEADER = "taxid;name;rank;parent taxid;tp;tp+fp;tp+fn;precision;recall;weighted avg precision;weighted avg recall;"


def pack(parts):
    """list of bytes -> (seq uint8, offsets uint64)"""
    seq = np.frombuffer(b"".join(parts), dtype=np.uint8)
    if len(seq) == 0:
        seq = np.zeros(1, dtype=np.uint8)
    return seq, np.cumsum([0] + [len(s) for s in parts]).astype(np.uint64)


def leaf_kmers(k, regions, lower=True, step=1, max_dust=-1):
    """distinct canonical k-mers (ascending int64) of a list of regions (bytes), formed as AbstractStoreFastaReader does"""
    b = orc.DbBuild(k, 1, np.array([-1], np.int32), lower, step, max_dust)
    seq, off = pack(list(regions))
    b.fill(seq, off, np.zeros(len(regions), np.int32))
    b.optimize()
    kmers, _ = b.fetch()
    b.close()
    return kmers


def stored_pairs(store_kmers, store_vals, parent_vi):
    """what the store serves: the pairs whose value has a tree node, ascending (the k-mers are expected canonical)"""
    parent = np.asarray(parent_vi, dtype=np.int64)
    sk = np.asarray(store_kmers, dtype=np.int64)
    sv = np.asarray(store_vals, dtype=np.int64)
    keep = parent[sv] != -2
    sk, sv = sk[keep], sv[keep]
    o = np.argsort(sk, kind="stable")
    return sk[o], sv[o]


def reference_counts(k, store_kmers, store_vals, parent_vi, regions, lower=True, step=1, max_dust=-1, lo=None, hi=None):
    """regions: list of (bytes, leaf_vi).  -> dict(counts int64[n_values, 3] = tp, tp+fp, tp+fn; present uint8[n_values];
    distinct: {leaf: number of distinct k-mers of the leaf's genomes (in [lo, hi))})"""
    parent = np.asarray(parent_vi, dtype=np.int64)
    nv = len(parent)
    sk, sv = stored_pairs(store_kmers, store_vals, parent)
    per_value = np.bincount(sv, minlength=nv).astype(np.int64)
    counts = np.zeros((nv, 3), dtype=np.int64)
    present = np.zeros(nv, dtype=np.uint8)
    distinct = {}
    by_leaf = {}
    for s, leaf in regions:
        if leaf < 0 or parent[leaf] == -2:
            continue  # leafNode == null
        by_leaf.setdefault(int(leaf), []).append(s)
    for leaf, parts in sorted(by_leaf.items()):
        km = leaf_kmers(k, parts, lower, step, max_dust)
        if lo is not None:
            u = km.astype(np.uint64)
            km = km[(u >= np.uint64(lo)) & (u < np.uint64(hi))]
        distinct[leaf] = len(km)
        at = np.searchsorted(sk, km)
        at_c = np.minimum(at, max(len(sk) - 1, 0))
        found = (at < len(sk)) & (sk[at_c] == km) if len(sk) else np.zeros(len(km), bool)
        vals = sv[at_c[found]]
        path = set()
        a = leaf
        while a >= 0:
            path.add(a)
            a = int(parent[a])
        tp_fn = int(found.sum())
        if tp_fn == 0:
            continue
        present[leaf] = 1
        counts[leaf, 0] = int(np.isin(vals, np.fromiter(path, dtype=np.int64)).sum())
        counts[leaf, 1] = int(sum(per_value[a] for a in path))
        counts[leaf, 2] = tp_fn
    return dict(counts=counts, present=present, distinct=distinct)


def tree_order(parent_vi, position=None):
    """value indices with a node in tree iteration order: ascending position, pre-order (children by value index) when None"""
    parent = [int(p) for p in parent_vi]
    nodes = [v for v in range(len(parent)) if parent[v] != -2]
    if position is not None:
        return sorted(nodes, key=lambda v: position[v])
    kids = {v: [] for v in nodes}
    roots = []
    for v in nodes:
        (kids[parent[v]] if parent[v] >= 0 else roots).append(v)
    out, stack = [], roots[::-1]
    while stack:
        v = stack.pop()
        out.append(v)
        stack.extend(kids[v][::-1])
    return out


class _Counts:
    def __init__(self, tp=0, tp_fp=0, tp_fn=0):
        self.tp, self.tp_fp, self.tp_fn = int(tp), int(tp_fp), int(tp_fn)
        self.aggregations, self.psum, self.rsum = 0, 0.0, 0.0

    @staticmethod
    def _div(a, b):
        return a / b if b else (float("nan") if a == 0 else float("inf"))

    def precision(self):
        return self._div(self.tp, self.tp_fp)

    def recall(self):
        return self._div(self.tp, self.tp_fn)

    def avg_precision(self):
        return self.precision() if self.psum == 0 else self.psum / self.aggregations

    def avg_recall(self):
        return self.recall() if self.rsum == 0 else self.rsum / self.aggregations

    def aggregate(self, c):
        self.tp += c.tp
        self.tp_fp += c.tp_fp
        self.tp_fn += c.tp_fn
        self.aggregations += 1
        self.psum += c.avg_precision()
        self.rsum += c.avg_recall()


def _df8(x):
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "∞" if x > 0 else "-∞"
    return format(x, ".8f")


def quality_csv(parent_vi, taxids, counts, present, names=None, ranks=None, position=None):
    """the CSV as bytes"""
    parent = [int(p) for p in parent_vi]
    order = tree_order(parent, position)
    own = {v: _Counts(*counts[v]) for v in order if present[v]}
    agg = {}
    for v in order:
        if v not in own or ranks is None:
            continue
        for rank in AGG_RANKS:
            a = v
            while a >= 0 and ranks[a] != rank:
                a = parent[a]
            if a >= 0 and a not in own:
                agg.setdefault(a, _Counts()).aggregate(own[v])
    rows = dict(own)
    rows.update(agg)
    lines = [HEADER]
    for v in order:
        c = rows.get(v)
        if c is None:
            continue
        name = "null" if names is None or names[v] is None else names[v]
        rank = "" if ranks is None or ranks[v] is None else ranks[v]
        par = taxids[parent[v]] if parent[v] >= 0 else "null"
        lines.append(f"{taxids[v]};{name};{rank};{par};{c.tp};{c.tp_fp};{c.tp_fn};{_df8(c.avg_precision())};{_df8(c.avg_recall())};"
                     f"{_df8(c.precision())};{_df8(c.recall())};")
    return ("\n".join(lines) + "\n").encode("utf-8")
