"""gs_taxtree_regions_below on the device (gs_taxtree.hip: regions scattered to pre-order, one scan, a difference per node; the
selection marked, flagged, scanned and compacted) against the hand-worked cases and, on generated trees, against the plain-Python
restatement (tests/assembly.py): regions in host and in device memory, from arrays and from a real accession map; node counts below,
at and above one block of the kernels; components the root does not reach; a tree that lives on the host after duplicate ids.
Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import assembly
import genestrip_amd as ga
import taxtree
from accmap_cases import CFG
from accmap_cases import L as CL
from assembly_cases import REGIONS_CASES, generated
from taxtree_cases import random_dump

pytestmark = pytest.mark.gpu


def reference(nodes):
    return taxtree.Tree(taxtree.nodes_slots(nodes))


def device_tree(nodes):
    t = ga.DeviceTaxTree()
    assert t.submit_nodes(nodes, last=True)["refused"] == 0
    t.finish()
    return t


def case_arrays(ref, by_taxid):
    out = np.zeros(ref.n, dtype=np.int32)
    for taxid, count in by_taxid.items():
        out[ref.node_of(taxid)] = count
    return out


def both_memories(regions):
    import torch

    return (regions, torch.from_numpy(regions).to("cuda"))


@pytest.mark.parametrize("name", sorted(REGIONS_CASES))
def test_hand_worked_counts(name):
    nodes, regions, inclusive, queries = REGIONS_CASES[name]
    ref = reference(nodes)
    t = device_tree(nodes)
    assert t.on_host == (name == "duplicate_id") and t.device == 0
    for r in both_memories(case_arrays(ref, regions)):
        if inclusive is None:
            with pytest.raises(ga.GsError) as e:
                t.regions_below(r, [0], 1)
            assert e.value.code == -1 and "cycle" in str(e.value)
            continue
        for selected, limit, rank, want in queries + [([], 1, None, [])]:
            below, incl = t.regions_below(r, [ref.node_of(i) for i in selected], limit, rank)
            assert incl.tolist() == case_arrays(ref, inclusive).tolist()
            assert ref.taxids[below].tolist() == want, (selected, limit, rank)


# 249 + 7 nodes are one block of the kernels exactly, 248 and 250 one below and one above it; 3000: several blocks
@pytest.mark.parametrize("n", [248, 249, 250, 3000])
def test_generated_trees_with_unreached_components(n):
    nodes, regions = generated(n, seed=60 + n % 7)
    ref = reference(nodes)
    assert ref.n == n + 7 == len(regions) and (ref.position[-7:] == -1).all() and (ref.position[:-7] >= 0).all()
    t = device_tree(nodes)
    assert t.on_host == 0 and t.n_reached == n
    want = assembly.regions_inclusive(ref.parent, regions)
    assert want[ref.root] == regions[:-7].sum()
    selected = ref.select([ref.root, ref.n - 6, ref.n - 3], [], taxtree.RANK_NAMES.index("species"))
    idx = np.flatnonzero(selected)
    for r in both_memories(regions):
        for limit, rank in ((1, None), (30, None), (30, "species"), (2 ** 31 - 1, None)):
            below, incl = t.regions_below(r, selected, limit, rank)
            assert np.array_equal(incl, want)
            expect = assembly.regions_below(ref.rank, want, idx, limit, None if rank is None else taxtree.RANK_NAMES.index(rank))
            assert below.tolist() == expect
            if limit == 30:
                assert 0 < len(expect) < len(idx)
        # indices in any order and with repeats: once each, ascending
        assert t.regions_below(r, np.concatenate([idx[::-1], idx[:5]]), 30)[0].tolist() == assembly.regions_below(ref.rank, want, idx, 30)


def test_a_tree_the_root_reaches_whole():
    """no host step in between: every node is reached (the shape of a real dump); a chain as deep as it has nodes beside it"""
    for nodes in (random_dump(2560, seed=71), b"".join(b"%d\t|\t%d\t|\t%s\t|\n" % (i, max(i - 1, 1), b"species" if i % 2 else b"genus") for i in range(1, 601))):
        ref = reference(nodes)
        assert (ref.position >= 0).all()
        t = device_tree(nodes)
        regions = np.where(np.arange(ref.n) % 5 == 0, 3, 0).astype(np.int32)
        want = assembly.regions_inclusive(ref.parent, regions)
        launches = t.kernel_time(True)[0]
        for r in both_memories(regions):
            below, incl = t.regions_below(r, np.arange(ref.n), 10, "species")
            assert np.array_equal(incl, want)
            assert below.tolist() == assembly.regions_below(ref.rank, want, range(ref.n), 10, taxtree.RANK_NAMES.index("species")) and len(below) > 0
        assert t.kernel_time(False)[0] == launches + 4  # per call: the counts, and the selection


def test_regions_of_a_real_accession_map():
    """dump -> tree -> taxnodes -> catalog -> accession map -> its regions, fetched and on the way there -> the nodes short of genomes"""
    nodes = random_dump(3000, seed=73, max_id=50000)
    ref = reference(nodes)
    t = device_tree(nodes)
    a = t.arrays()
    species = taxtree.RANK_NAMES.index("species")
    selected = t.select([ref.root], [], "species")
    assert np.array_equal(selected, ref.select([ref.root], [], species))
    rng = np.random.default_rng(74)
    # accessions at every third node, one to six each, at selected nodes and below them alike
    at = np.repeat(np.arange(0, ref.n, 3), rng.integers(1, 7, size=len(range(0, ref.n, 3))))
    catalog = b"".join(CL(str(int(a["taxids"][v])), f"NC_{i:06d}.1") for i, v in enumerate(at))
    m = ga.DeviceAccessionMap(a["taxids"], CFG["categories"], CFG["statuses"], CFG["seq_type"])
    assert m.submit(catalog, last=True)["refused"] == 0
    m.finish()
    regions = m.fetch()[2]
    assert np.array_equal(regions, np.bincount(at, minlength=ref.n))
    want = assembly.regions_inclusive(ref.parent, regions)
    assert want[ref.root] == len(at)
    for r in both_memories(regions.astype(np.int32)):
        below, incl = t.regions_below(r, selected, 4, "species")
        assert np.array_equal(incl, want)
        expect = assembly.regions_below(ref.rank, want, np.flatnonzero(selected), 4, species)
        assert below.tolist() == expect and 0 < len(expect) < int((ref.rank[selected > 0] == species).sum())
    # per-node counts alone would call more nodes short than the goal does
    assert len(expect) < len(assembly.regions_below(ref.rank, regions, np.flatnonzero(selected), 4, species))
