"""The taxfromgenbank goal in plain Python, written from the reference's Java: TaxIdNode.incRefSeqRegions (C/tax/TaxTree.java:517-521),
called once per entry that AccessionMapGoal puts (C/goals/refseq/AccessionMapGoal.java:96-102), and the loop of
TaxNodesFromGenbankGoal.doMakeThis (C/goals/genbank/TaxNodesFromGenbankGoal.java:73-97).

A node is its index in the ascending array of distinct tax ids (tests/taxtree.py).  `regions` counts the entries of the accession map
per node ITSELF, as gs_accmap_fetch gives them; the reference keeps the count with everything below the node, which is what
regions_inclusive makes of them.  The reference's result is a HashSet; here it is a list in ascending node index."""
import numpy as np

from taxtree import Throws


def regions_inclusive(parent, regions):
    """incRefSeqRegions per entry: every entry of node v counts for v and for each node on its parent chain -> int64[n].
    A node with entries on or below a cycle of parent links: the reference's loop does not end"""
    n = len(parent)
    incl = np.zeros(n, dtype=np.int64)
    for v in np.flatnonzero(np.asarray(regions)):
        count, u, steps = int(regions[v]), int(v), 0
        while u != -1:
            if steps > n:
                raise Throws(0, "incRefSeqRegions does not end: a cycle of parent links")
            incl[u] += count
            u = int(parent[u])
            steps += 1
    return incl


def regions_below(rank, inclusive, selected, limit, check_rank=None, refseq_db=True, rna_only=False):
    """TaxNodesFromGenbankGoal.doMakeThis over node indices: selected is the taxnodes set, limit refSeq.limitForGenbankAccess,
    check_rank the ordinal of refSeq.limitForGenbankRank or None -> the sorted list of the missing nodes"""
    missing = set()
    if not refseq_db:
        missing.update(int(v) for v in selected)
    elif not rna_only:
        if limit > 0:
            for v in selected:
                if check_rank is None or check_rank == int(rank[v]):  # (a node without a rank: Rank.equals(null) is false)
                    if int(inclusive[v]) < limit:
                        missing.add(int(v))
    return sorted(missing)
