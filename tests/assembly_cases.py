"""Hand-worked cases of the taxfromgenbank goal: every expected value below is typed in, none is computed.  Nodes are named by
their tax ids; the tests turn them into node indices (the index in the ascending array of distinct ids)."""
import numpy as np

from taxtree_cases import L, random_dump

# name -> (nodes lines, {tax id: entries of the accession map at that node itself},
#          {tax id: entries at the node and below it}, or None where the reference's walk does not end,
#          [(selected tax ids, limit, rank to check or None, the selected ids that come out)])
REGIONS_CASES = {
    # five levels, entries at the leaf alone: every level counts them
    "chain_leaf_only": (
        L(1, 1) + L(2, 1, "superkingdom") + L(3, 2, "genus") + L(4, 3, "species") + L(5, 4, "strain"),
        {5: 3},
        {1: 3, 2: 3, 3: 3, 4: 3, 5: 3},
        [([3, 4, 5], 4, None, [3, 4, 5]), ([3, 4, 5], 3, None, []), ([5, 3, 4, 3], 4, "species", [4]), ([], 4, None, []),
         ([1, 2, 3, 4, 5], 2147483647, None, [1, 2, 3, 4, 5])]),
    # siblings whose sums straddle the limit; 31 has a rank that is none of Rank's
    "siblings": (
        L(1, 1) + L(10, 1, "genus") + L(11, 10, "species") + L(12, 10, "species") + L(13, 10, "species") + L(20, 11, "strain") + L(21, 11, "strain") +
        L(22, 12, "strain") + L(30, 1, "species") + L(31, 1, "weird"),
        {10: 1, 11: 1, 12: 3, 13: 5, 20: 2, 21: 1},
        {1: 13, 10: 13, 11: 4, 12: 3, 13: 5, 20: 2, 21: 1, 22: 0, 30: 0, 31: 0},
        [([10, 11, 12, 13, 20, 21, 22, 30, 31], 4, None, [12, 20, 21, 22, 30, 31]),
         ([10, 11, 12, 13, 20, 21, 22, 30, 31], 4, "species", [12, 30]),
         ([10, 11, 12, 13, 20, 21, 22, 30, 31], 4, "strain", [20, 21, 22]),
         ([31, 30, 22, 21, 20, 13, 12, 11, 10], 5, "species", [11, 12, 30]),
         ([10, 11, 12, 13], 14, None, [10, 11, 12, 13]),
         ([10, 11, 12, 13], 13, "genus", []),
         ([10, 11, 12, 13], 14, "genus", [10]),
         ([1], 13, None, []),
         ([11, 13], 1, None, [])]),
    # what the root does not reach: 60 is named as a parent alone, 70 is a second node that is its own parent
    "unreached": (
        L(1, 1) + L(2, 1, "species") + L(50, 60, "species") + L(51, 50, "strain") + L(70, 70) + L(71, 70, "species"),
        {2: 1, 50: 1, 51: 2, 71: 4},
        {1: 1, 2: 1, 50: 3, 51: 2, 60: 3, 70: 4, 71: 4},
        [([2, 50, 51, 60, 70, 71], 4, None, [2, 50, 51, 60]), ([2, 50, 51, 60, 70, 71], 4, "species", [2, 50]), ([70, 71], 5, None, [70, 71])]),
    # two lines with one id: the node keeps the parent of its last line
    "duplicate_id": (
        L(1, 1) + L(2, 1, "genus") + L(3, 2, "species") + L(3, 1, "species"),
        {3: 2},
        {1: 2, 2: 0, 3: 2},
        [([2, 3], 1, None, [2]), ([2, 3], 3, "species", [3])]),
    # entries on a cycle, and on a node that hangs below one
    "cycle_with_entries": (L(1, 1) + L(80, 82, "genus") + L(82, 80, "genus") + L(84, 82, "species"), {82: 1}, None, []),
    "below_a_cycle_with_entries": (L(1, 1) + L(80, 82, "genus") + L(82, 80, "genus") + L(84, 82, "species"), {84: 1}, None, []),
    # a cycle without entries is walked by nobody
    "cycle_without_entries": (
        L(1, 1) + L(2, 1, "species") + L(80, 82, "genus") + L(82, 80, "genus") + L(84, 82, "species"),
        {2: 2},
        {1: 2, 2: 2, 80: 0, 82: 0, 84: 0},
        [([2, 80, 84], 1, None, [80, 84])]),
}


def generated(n, seed):
    """a dump of n nodes under the root in shuffled line order, with components the root does not reach -> (nodes lines,
    regions per node: most nodes none, some many)"""
    top = 40 * n
    extra = (L(top + 1, top + 2, "species") + L(top + 3, top + 1, "strain") + L(top + 4, top + 1, "strain") + L(top + 7, top + 7) + L(top + 8, top + 7, "genus") +
             L(top + 9, top + 8, "species"))
    nodes = random_dump(n, seed) + extra
    rng = np.random.default_rng(seed + 1000)
    n_nodes = n + 7  # (top + 2 is a node as well)
    regions = np.where(rng.random(n_nodes) < 0.3, rng.integers(1, 40, n_nodes), 0).astype(np.int32)
    regions[-7:] = [2, 0, 5, 1, 0, 3, 7]
    return nodes, regions
