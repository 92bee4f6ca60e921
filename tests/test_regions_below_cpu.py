"""The taxfromgenbank goal without a GPU: the plain-Python restatement (tests/assembly.py) against the hand-worked cases, and
gs_taxtree_regions_below under the host-only handle (device -1) against the cases and, on generated trees, against the restatement."""
import ctypes as C

import numpy as np
import pytest

import assembly
import genestrip_amd as ga
import taxtree
from assembly_cases import REGIONS_CASES, generated


def reference(nodes):
    return taxtree.Tree(taxtree.nodes_slots(nodes))


def host_tree(nodes, pieces=1):
    t = ga.DeviceTaxTree(device=-1)
    cuts = [0] + [nodes.rfind(b"\n", 0, len(nodes) * i // pieces) + 1 for i in range(1, pieces)] + [len(nodes)]
    for a, b in zip(cuts, cuts[1:]):
        t.append_nodes(nodes[a:b], last=b == len(nodes))
    t.finish()
    return t


def case_arrays(ref, by_taxid):
    out = np.zeros(ref.n, dtype=np.int32)
    for taxid, count in by_taxid.items():
        out[ref.node_of(taxid)] = count
    return out


def rank_ordinal(name):
    return None if name is None else taxtree.RANK_NAMES.index(name)


# (this test checks the restatement itself against the values typed in and touches no symbol of the library)
@pytest.mark.parametrize("name", sorted(REGIONS_CASES))
def test_restatement_gives_the_hand_worked_counts(name):
    nodes, regions, inclusive, queries = REGIONS_CASES[name]
    ref = reference(nodes)
    assert set(inclusive or regions) <= set(ref.taxids.tolist())
    if inclusive is None:
        with pytest.raises(taxtree.Throws):
            assembly.regions_inclusive(ref.parent, case_arrays(ref, regions))
        return
    assert len(inclusive) == ref.n  # every node has its typed value
    incl = assembly.regions_inclusive(ref.parent, case_arrays(ref, regions))
    assert incl.tolist() == case_arrays(ref, inclusive).tolist()
    for selected, limit, rank, want in queries:
        got = assembly.regions_below(ref.rank, incl, [ref.node_of(t) for t in selected], limit, rank_ordinal(rank))
        assert ref.taxids[got].tolist() == want, (selected, limit, rank)


@pytest.mark.parametrize("name", sorted(REGIONS_CASES))
def test_host_only_handle_gives_the_hand_worked_counts(name):
    nodes, regions, inclusive, queries = REGIONS_CASES[name]
    ref = reference(nodes)
    t = host_tree(nodes)
    if inclusive is None:
        with pytest.raises(ga.GsError) as e:
            t.regions_below(case_arrays(ref, regions), [0], 1)
        assert e.value.code == -1 and "cycle" in str(e.value)
        return
    for selected, limit, rank, want in queries + [([], 1, None, [])]:
        below, incl = t.regions_below(case_arrays(ref, regions), [ref.node_of(i) for i in selected], limit, rank)
        assert incl.tolist() == case_arrays(ref, inclusive).tolist()
        assert ref.taxids[below].tolist() == want, (selected, limit, rank)


@pytest.mark.parametrize("seed", [51, 52, 53])
def test_host_only_handle_on_generated_trees(seed):
    nodes, regions = generated(2000, seed)
    ref = reference(nodes)
    assert ref.n == len(regions) and (ref.position[-7:] == -1).all() and (ref.position[:-7] >= 0).all()
    t = host_tree(nodes, pieces=3)
    want = assembly.regions_inclusive(ref.parent, regions)
    assert want[ref.root] == regions[:-7].sum() and want.max() < 2 ** 31
    selected = ref.select([ref.root, ref.n - 6, ref.n - 3], [], taxtree.RANK_NAMES.index("species"))
    for limit, rank in ((1, None), (30, None), (30, "species"), (200, "genus"), (2 ** 31 - 1, None)):
        below, incl = t.regions_below(regions, selected, limit, rank)
        assert np.array_equal(incl, want)
        expect = assembly.regions_below(ref.rank, want, np.flatnonzero(selected), limit, rank_ordinal(rank))
        assert below.tolist() == expect
        if limit == 30:  # (a limit that cuts the selection in two)
            assert 0 < len(expect) < selected.sum(), (rank, len(expect))
    # the same selection as indices in any order and with repeats: once each, ascending
    idx = np.flatnonzero(selected)
    shuffled = np.concatenate([idx[::-1], idx[:5]])
    assert t.regions_below(regions, shuffled, 30)[0].tolist() == assembly.regions_below(ref.rank, want, idx, 30)


def test_what_the_goal_puts_in_front():
    nodes, regions, inclusive, _ = REGIONS_CASES["siblings"]
    ref = reference(nodes)
    t = host_tree(nodes)
    r = case_arrays(ref, regions)
    sel = [ref.node_of(i) for i in (13, 12, 11, 12)]
    ids = lambda got: ref.taxids[got[0]].tolist()
    assert ids(t.regions_below(r, sel, 4)) == [12]
    assert ids(t.regions_below(r, sel, 4, refseq_db=False)) == [11, 12, 13]  # without refseq.filldb: the whole selection
    assert ids(t.regions_below(r, sel, 4, rna_only=True)) == []
    assert ids(t.regions_below(r, sel, 0)) == [] and ids(t.regions_below(r, sel, -3)) == []
    for kw in ({}, {"refseq_db": False}, {"rna_only": True}):
        assert assembly.regions_below(ref.rank, case_arrays(ref, inclusive), sel, 4, **kw) == sorted(set(t.regions_below(r, sel, 4, **kw)[0].tolist()))
    assert t.regions_below(r, sel, 4)[1].tolist() == case_arrays(ref, inclusive).tolist()


def test_argument_and_state_errors():
    L = ga.lib()
    nodes = REGIONS_CASES["siblings"][0]
    ref = reference(nodes)
    o = (C.c_int32 * 16)()
    sel = (C.c_int32 * 2)(1, 2)
    n = C.c_int64()
    assert L.gs_taxtree_regions_below(None, o, 0, sel, 2, 4, -1, None, None, None) == -1
    h = C.c_void_p()
    assert L.gs_taxtree_create(C.byref(h), -1) == 0
    assert L.gs_taxtree_regions_below(h, o, 0, sel, 2, 4, -1, None, None, None) == -5  # in front of the finish
    L.gs_taxtree_destroy(h)
    t = host_tree(nodes)
    assert L.gs_taxtree_regions_below(t.h, None, 0, sel, 2, 4, -1, None, None, None) == -1
    assert L.gs_taxtree_regions_below(t.h, o, 0, None, 2, 4, -1, None, None, None) == -1
    assert L.gs_taxtree_regions_below(t.h, o, 0, sel, -1, 4, -1, None, None, None) == -1
    assert L.gs_taxtree_regions_below(t.h, o, 0, sel, 2, 4, -2, None, None, None) == -1
    assert L.gs_taxtree_regions_below(t.h, o, 0, sel, 2, 4, len(taxtree.RANK_NAMES), None, None, None) == -1
    assert L.gs_taxtree_regions_below(t.h, o, 2, sel, 2, 4, -1, None, None, None) == -1
    assert L.gs_taxtree_regions_below(t.h, o, 1, sel, 2, 4, -1, None, None, None) == -4  # a host-only tree reads host memory alone
    bad = (C.c_int32 * 2)(1, ref.n)
    assert L.gs_taxtree_regions_below(t.h, o, 0, bad, 2, 4, -1, None, None, None) == -1
    o[3] = -1
    assert L.gs_taxtree_regions_below(t.h, o, 0, sel, 2, 4, -1, None, None, None) == -1  # a negative count
    o[3] = 0
    # every output may be NULL, and none of them alone is needed
    assert L.gs_taxtree_regions_below(t.h, o, 0, sel, 2, 4, -1, None, None, None) == 0
    assert L.gs_taxtree_regions_below(t.h, o, 0, None, 0, 4, -1, None, None, C.byref(n)) == 0 and n.value == 0
    assert L.gs_taxtree_regions_below(t.h, o, 0, sel, 2, 4, -1, None, None, C.byref(n)) == 0 and n.value == 2
    with pytest.raises(ValueError):
        t.regions_below(np.zeros(ref.n + 1, dtype=np.int32), [0], 1)
