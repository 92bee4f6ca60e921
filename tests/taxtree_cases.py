"""Hand-worked cases of the taxtree and taxnodes goals, each with what it must give, read off the reference's Java (the places are
named in tests/taxtree.py), and the generators of the larger dumps.  A case: (nodes bytes, expected) where expected is a dict of
the arrays, ("throws", 1-based line) or ("unsupported", 1-based line).  IN_GRAMMAR names the cases the device takes as they are."""
import os

import numpy as np

import taxtree
from conftest import GOLDEN

R = taxtree.RANK_NAMES.index


def L(tid, parent, rank="no rank", nl="\n", rest="\t|\t\t|"):
    return f"{tid}\t|\t{parent}\t|\t{rank}{rest}{nl}".encode()


def _sized(size, tid=2, parent=1, rank="species"):
    """a line of exactly `size` bytes with its newline"""
    head = f"{tid}\t|\t{parent}\t|\t{rank}\t|\t".encode()
    return head + b"x" * (size - len(head) - 1) + b"\n"


def _arr(taxids, parent, depth, position, subtree, rank):
    return {k: np.array(v, dtype=np.int32) for k, v in zip(("taxids", "parent", "depth", "position", "subtree", "rank"),
                                                           (taxids, parent, depth, position, subtree, rank))}


with open(os.path.join(GOLDEN, "taxtree", "nodes.dmp"), "rb") as _f:
    GOLDEN_NODES = _f.read()
with open(os.path.join(GOLDEN, "taxtree", "names.dmp"), "rb") as _f:
    GOLDEN_NAMES = _f.read()

NR, SP, GE = R("no rank"), R("species"), R("genus")
_TWO = _arr([1, 2], [-1, 0], [0, 1], [0, 1], [2, 1], [NR, SP])
CASES = {
    "golden": (GOLDEN_NODES, _arr([1, 2, 3], [-1, 0, 0], [0, 1, 1], [0, 1, 2], [3, 1, 1], [NR] * 3)),
    # a line with one bar is skipped
    "one_bar": (L(1, 1) + b"5\t|\n" + L(2, 1, "species"), _TWO),
    # two bars and no third: c == -1, the rank compares a negative length: none
    "two_bars": (L(1, 1) + b"2\t|\t1\t|\n", _arr([1, 2], [-1, 0], [0, 1], [0, 1], [2, 1], [NR, -1])),
    "empty_line": (L(1, 1) + b"\n" + L(2, 1, "species"), _TWO),
    "no_final_newline": (L(1, 1) + L(2, 1, "species", nl=""), _TWO),
    "crlf": (L(1, 1, nl="\r\n") + L(2, 1, "species", nl="\r\n"), _TWO),
    # NUL bytes are dropped: the id is 20
    "nul_in_id": (L(1, 1) + b"2\x000\t|\t1\t|\tspecies\t|\n", _arr([1, 20], [-1, 0], [0, 1], [0, 1], [2, 1], [NR, SP])),
    "unknown_rank": (L(1, 1) + L(2, 1, "superduper") + L(3, 1, "Species") + L(4, 1, ""),
                     _arr([1, 2, 3, 4], [-1, 0, 0, 0], [0, 1, 1, 1], [0, 1, 2, 3], [4, 1, 1, 1], [NR, -1, -1, -1])),
    "every_rank": (L(1, 1) + b"".join(L(i + 2, 1, name) for i, name in enumerate(taxtree.RANK_NAMES)),
                   _arr(range(1, 42), [-1] + [0] * 40, [0] + [1] * 40, range(41), [41] + [1] * 40, [NR] + list(range(40)))),
    "leading_zero": (L(1, 1) + L("02", 1), ("unsupported", 2)),
    "empty_id": (L(1, 1) + b"\t|\t1\t|\tspecies\t|\n", ("unsupported", 2)),
    "no_digit": (L(1, 1) + L(3, 1) + L("2a", 1), ("throws", 3)),
    "bar_first": (L(1, 1) + b"|\t1\t|\tspecies\t|\n", ("throws", 2)),
    # a parent that no line introduces is a node: no rank, no parent; the root does not reach it
    "parent_only": (L(1, 1) + L(3, 7, "species"), _arr([1, 3, 7], [-1, 2, -1], [0, -1, -1], [0, -1, -1], [1, 0, 0], [NR, SP, -1])),
    "second_self_parent": (L(1, 1) + L(5, 5) + L(6, 5, "species") + L(2, 1, "genus"),
                           _arr([1, 2, 5, 6], [-1, 0, -1, 2], [0, 1, -1, -1], [0, 1, -1, -1], [2, 1, 0, 0], [NR, GE, NR, SP])),
    "two_cycle": (L(1, 1) + L(2, 1, "genus") + L(8, 9) + L(9, 8) + L(10, 9, "species"),
                  _arr([1, 2, 8, 9, 10], [-1, 0, 3, 2, 3], [0, 1, -1, -1, -1], [0, 1, -1, -1, -1], [2, 1, 0, 0, 0], [NR, GE, NR, NR, SP])),
    # two lines with one id: the node is listed twice and walked twice; the last visit stays
    "dup_same_parent": (L(1, 1) + L(2, 1, "genus") + L(2, 1, "genus") + L(3, 2, "species"),
                        _arr([1, 2, 3], [-1, 0, 1], [0, 1, 2], [0, 3, 4], [5, 2, 1], [NR, GE, SP])),
    "dup_other_parent": (L(1, 1) + L(2, 1, "genus") + L(3, 1, "genus") + L(2, 3, "species"),
                         _arr([1, 2, 3], [-1, 2, 0], [0, 2, 1], [0, 3, 2], [4, 1, 2], [NR, SP, GE])),
    "line_4095": (L(1, 1) + _sized(4095) + L(3, 2, "strain"), _arr([1, 2, 3], [-1, 0, 1], [0, 1, 2], [0, 1, 2], [3, 2, 1], [NR, SP, R("strain")])),
    "line_4096": (L(1, 1) + _sized(4096) + L(3, 2, "strain"), _arr([1, 2, 3], [-1, 0, 1], [0, 1, 2], [0, 1, 2], [3, 2, 1], [NR, SP, R("strain")])),
    # 4097 bytes: the line is its first 4096, the newline alone is the next line (skipped)
    "line_4097": (L(1, 1) + _sized(4097) + L(3, 2, "strain"), _arr([1, 2, 3], [-1, 0, 1], [0, 1, 2], [0, 1, 2], [3, 2, 1], [NR, SP, R("strain")])),
    # ... and a rest that is a line of its own is read as one
    "line_split_rest": (L(1, 1) + _sized(4097)[:-1] + L(3, 1, "genus"), _arr([1, 2, 3], [-1, 0, 0], [0, 1, 1], [0, 1, 2], [3, 1, 1], [NR, SP, GE])),
    # a line that fills the buffer without a third bar: the search reads behind it
    "line_long_no_bars": (L(1, 1) + b"2\t|\t1\t|" + b"x" * 5000 + b"\n", ("throws", 2)),
    "no_root": (L(2, 1) + L(3, 2), ("throws", 0)),
    "root_not_self": (L(1, 2) + L(2, 2), ("throws", 0)),
    "cycle_under_root_by_duplicates": (L(1, 1) + L(2, 1) + L(3, 2) + L(2, 3), ("throws", 0)),
}
IN_GRAMMAR = ("golden", "empty_line", "no_final_newline", "crlf", "unknown_rank", "every_rank", "parent_only", "second_self_parent",
              "two_cycle", "dup_same_parent", "dup_other_parent", "line_4095", "line_4096", "no_root", "root_not_self",
              "cycle_under_root_by_duplicates")
# the first line outside the grammar, 0-based, of the others
FIRST_BAD = {"one_bar": 1, "two_bars": 1, "nul_in_id": 1, "leading_zero": 1, "empty_id": 1, "no_digit": 2, "bar_first": 1, "line_4097": 1,
             "line_split_rest": 1, "line_long_no_bars": 1}

# ---- names: over the tree of NAMES_NODES; expected names per node, ascending ids 1, 2, 3, 4
NAMES_NODES = L(1, 1) + L(2, 1, "genus") + L(3, 2, "species") + L(4, 2, "species")


def N(tid, name, kind="synonym", nl="\n"):
    return f"{tid}\t|\t{name}\t|\t\t|\t{kind}\t|{nl}".encode()


NAMES_CASES = {
    "golden": (GOLDEN_NODES, GOLDEN_NAMES, [b"1", b"2", b"3"]),
    "unknown_id": (NAMES_NODES, N(1, "root", "scientific name") + N(77, "nobody") + N("x7", "nobody") + N("01", "nobody"), [b"root", None, None, None]),
    "two_scientific": (NAMES_NODES, N(2, "Old", "scientific name") + N(2, "New", "scientific name"), [None, b"New", None, None]),
    # the search runs over the whole line: a synonym whose NAME holds the words replaces the name
    "scientific_inside_name": (NAMES_NODES, N(3, "Real", "scientific name") + N(3, "not a scientific name at all"), [None, None, b"not a scientific name at all", None]),
    "synonym_before_and_after": (NAMES_NODES, N(4, "First") + N(4, "Second") + N(4, "Sci", "scientific name") + N(4, "Third"), [None, None, None, b"Sci"]),
    "first_synonym_wins": (NAMES_NODES, N(4, "First") + N(4, "Second"), [None, None, None, b"First"]),
    "utf8": (NAMES_NODES, N(2, "Café 中文", "scientific name"), [None, "Café 中文".encode(), None, None]),
    "one_bar_and_crlf": (NAMES_NODES, b"2\t|\n" + N(2, "Crlf", nl="\r\n"), [None, b"Crlf", None, None]),
    "no_final_newline": (NAMES_NODES, N(3, "Tail", nl=""), [None, None, b"Tail", None]),
    "negative_name": (NAMES_NODES, N(3, "ok") + b"2\t||\n", ("throws", 2)),
}

# ---- the tax id file
TAXIDS_TEXT = (b"# a comment\n\n  9606  \nhuman\t9606\n-562 # an exclude\nname\tmore\t 10090\n#-7\n12x\n007\n-\n   \t-11 \r\n1234567890\n4932#x\n77")
TAXIDS_EXPECT = (["9606", "9606", "10090", "12x", "007", "1234567890", "4932", "77"], ["562", "", "11"])
TAXIDS_NUMBERS = ([9606, 9606, 10090, 4932, 77], [562, 11])  # what names a tax id of this library

# ---- selection: root 1 > 2 superkingdom > 3 no rank > 4 genus > 5 clade > 6 species > 7 (unknown rank: null) > 8 strain
#                                                       4 > 9 species > 10 strain;  6 > 11 no rank;  6 > 12 subspecies
SELECT_NODES = (L(1, 1) + L(2, 1, "superkingdom") + L(3, 2) + L(4, 3, "genus") + L(5, 4, "clade") + L(6, 5, "species") + L(7, 6, "weird") +
                L(8, 7, "strain") + L(9, 4, "species") + L(10, 9, "strain") + L(11, 6) + L(12, 6, "subspecies"))
# (requested ids, excluded ids, cut) -> the ids that are in
SELECT_CASES = {
    "no_cut": ([4], [], None, [4, 5, 6, 7, 8, 9, 10, 11, 12]),
    # no rank and clade are never below; a null rank and what is below species stop the descent
    "cut_species": ([2], [], "species", [2, 3, 4, 5, 6, 9, 11]),
    "cut_genus": ([2], [], "genus", [2, 3, 4, 5]),
    # the start node is added whatever its rank
    "requested_below_cut": ([10, 8], [], "species", [8, 10]),
    "requested_null_rank": ([7], [], "species", [7]),
    "exclude_inside": ([4], [6], None, [4, 5, 9, 10]),
    "exclude_outside_and_unknown": ([9], [2222, 5], "species", [9]),
    "exclude_all": ([6], [1], None, []),
    "two_requested_nested": ([2, 6], [], "genus", [2, 3, 4, 5, 6, 11]),
}


# ---- generated dumps
def random_dump(n, seed, shuffle=True, max_id=None):
    """n nodes under the root: a random parent among the nodes made before, ids drawn without order, ranks of every kind,
    lines in shuffled order"""
    rng = np.random.default_rng(seed)
    ids = np.concatenate([[1], 2 + rng.choice((max_id or 40 * n) - 2, size=n - 1, replace=False)])
    parent = np.concatenate([[0], (rng.random(n - 1) * np.arange(1, n) * rng.random(n - 1) ** 0.5).astype(np.int64)])
    ranks = ["no rank", "species", "genus", "strain", "clade", "family", "odd", "", "subspecies", "superkingdom", "forma specialis"]
    pick = rng.integers(0, len(ranks), size=n)
    lines = [L(int(ids[i]), int(ids[parent[i]]), ranks[pick[i]], rest="\t|\t\t|" if i % 3 else "\t|") for i in range(n)]
    if shuffle:
        lines = [lines[i] for i in rng.permutation(n)]
    return b"".join(lines)


def chain_dump(n):
    """1 <- 2 <- ... <- n, as deep as it has nodes"""
    return L(1, 1) + b"".join(L(i, i - 1, "species" if i % 2 else "no rank") for i in range(2, n + 1))


def star_dump(n):
    return L(1, 1) + b"".join(L(i, 1, "species") for i in range(n + 1, 1, -1))


def cuts_near(text, spots):
    """line boundaries of text next to every offset of spots, ascending, without 0 and len(text)"""
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10) + 1
    out = set()
    for s in spots:
        i = int(np.searchsorted(nl, s))
        for j in (i - 1, i):
            if 0 <= j < len(nl) and 0 < nl[j] < len(text):
                out.add(int(nl[j]))
    return sorted(out)
