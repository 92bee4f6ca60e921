"""The tree handle (gs_taxtree, genestrip_amd/csrc/gs_taxtree.hip) against the plain-Python restatement of the reference
(tests/taxtree.py): the scan's grammar and refusals, the arrays of the finish at every chunking, chains deeper than a block,
selection at every cut rank, the small tree, duplicate ids and call order."""
import numpy as np
import pytest

import genestrip_amd as ga
import taxtree
from taxtree_cases import (CASES, FIRST_BAD, IN_GRAMMAR, N, NAMES_CASES, SELECT_CASES, SELECT_NODES, chain_dump, cuts_near, random_dump, star_dump)

pytestmark = pytest.mark.gpu

KEYS = ("taxids", "parent", "depth", "position", "subtree", "rank")
_REF = {}


def reference(key, make):
    """one restatement per dump, shared and left unchanged"""
    if key not in _REF:
        nodes = make()
        _REF[key] = (nodes, taxtree.Tree(taxtree.nodes_slots(nodes)))
    return _REF[key]


def same(t, ref):
    got = t.arrays()
    for k in KEYS:
        assert np.array_equal(got[k], getattr(ref, k)), (k, got[k][:16], getattr(ref, k)[:16])


def device_tree(nodes, cuts=()):
    """the dump in chunks cut at `cuts`, every one of them taken by the device"""
    t = ga.DeviceTaxTree()
    edges = [0] + list(cuts) + [len(nodes)]
    for a, b in zip(edges, edges[1:]):
        rep = t.submit_nodes(nodes[a:b], last=b == len(nodes))
        lines = nodes[a:b].splitlines(keepends=True)
        assert rep == dict(lines=len(lines), taken=len(lines), refused=0, first_bad_line=-1, longest_line=max(map(len, lines))), (a, b, rep)
    return t


@pytest.mark.parametrize("name", sorted(n for n in IN_GRAMMAR if not isinstance(CASES[n][1], tuple)))
def test_hand_cases_inside_the_grammar(name):
    nodes, want = CASES[name]
    t = device_tree(nodes)
    info = t.finish()
    ref = taxtree.Tree(taxtree.nodes_slots(nodes))
    got = t.arrays()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert info["duplicates"] == ref.duplicates and info["on_host"] == (ref.duplicates > 0)
    assert info["reached"] == int((want["position"] >= 0).sum()) and info["max_depth"] == int(want["depth"].max())
    if name == "two_cycle":
        assert info["cycle_nodes"] == 2


@pytest.mark.parametrize("name", sorted(n for n in IN_GRAMMAR if isinstance(CASES[n][1], tuple)))
def test_trees_without_a_root_fail_at_finish(name):
    t = device_tree(CASES[name][0])
    with pytest.raises(ga.GsError) as e:
        t.finish()
    assert e.value.code == -1


@pytest.mark.parametrize("name", sorted(FIRST_BAD))
def test_hand_cases_outside_the_grammar_are_refused_and_appended(name):
    nodes, want = CASES[name]
    head = nodes[:nodes.index(b"\n") + 1]  # (every case starts with the root's line)
    assert head.startswith(b"1\t|\t1\t|\t")
    t = ga.DeviceTaxTree()
    assert t.submit_nodes(head)["taken"] == 1
    rest = nodes[len(head):]
    rep = t.submit_nodes(rest, last=True)
    assert rep["refused"] == 1 and rep["taken"] == 0 and rep["first_bad_line"] == FIRST_BAD[name] - 1, rep
    if isinstance(want, tuple):
        with pytest.raises(ga.GsError) as e:
            t.append_nodes(rest, last=True)
        assert e.value.code == (-1 if want[0] == "throws" else -4) and f"line {want[1]}:" in str(e.value)
        rest = b""  # the handle is as it was: the root alone
        want = CASES["golden"][1]
        want = {k: v[:1] if k != "subtree" else np.array([1], dtype=np.int32) for k, v in want.items()}
    else:
        t.append_nodes(rest, last=True)
    info = t.finish()
    assert info["on_host"] == 0
    got = t.arrays()
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


GENERATED = {"random": lambda: random_dump(5000, seed=11), "chain": lambda: chain_dump(3000), "star": lambda: star_dump(10000)}


@pytest.mark.parametrize("kind", sorted(GENERATED))
def test_generated_dumps_as_one_chunk_and_cut_near_tiles_and_lanes(kind):
    nodes, ref = reference(kind, GENERATED[kind])
    t = device_tree(nodes)
    info = t.finish()
    assert info == dict(nodes=ref.n, reached=ref.n, max_depth=int(ref.depth.max()), duplicates=0, on_host=0, cycle_nodes=0, slots=nodes.count(b"\n"))
    same(t, ref)
    # an id, a bar and a newline first, last and across a tile (4096 m +- 1) and a thread's 16 bytes (16 m +- 1): the cut moves
    # what follows it to offset 0
    # (every m of 4096 m +- 1; of 16 m +- 1 some 150 values of m spread over the text -- every one of them would cut at nearly every
    # line and make thousands of chunks; test_lines_that_straddle_tiles_and_lanes puts lines at every offset within 16 bytes)
    spots = [4096 * m + d for m in range(1, len(nodes) // 4096 + 1) for d in (-1, 0, 1)]
    step = max(len(nodes) // (16 * 150), 1)
    spots += [16 * m + d for m in range(1, len(nodes) // 16, step) for d in (-1, 1)]
    t = device_tree(nodes, cuts_near(nodes, spots))
    t.finish()
    same(t, ref)


def test_lines_that_straddle_tiles_and_lanes():
    """every alignment of a line against the 16 bytes of a thread, and lines across the tile's end: a filler line in front moves it"""
    root = CASES["golden"][0][:CASES["golden"][0].index(b"\n") + 1]
    parts, want = [root], []
    for i, shift in enumerate(list(range(0, 48)) + [4000 - d for d in range(0, 80, 3)]):
        parts.append(b"9%05d\t|\t1\t|\t" % i + b"y" * shift + b"\t|\n")
        parts.append(b"%d\t|\t9%05d\t|\tforma specialis\t|\tz\t|\n" % (100 + i, i))
    nodes = b"".join(parts)
    ref = taxtree.Tree(taxtree.nodes_slots(nodes))
    t = device_tree(nodes)
    t.finish()
    same(t, ref)


def test_a_chain_deeper_than_any_block():
    nodes, ref = reference("chain70000", lambda: chain_dump(70000))
    t = device_tree(nodes, cuts_near(nodes, [len(nodes) // 3, 2 * len(nodes) // 3]))
    info = t.finish()
    assert info["max_depth"] == 69999 and info["reached"] == 70000
    a = t.arrays()
    i = np.arange(70000, dtype=np.int32)
    assert np.array_equal(a["depth"], i) and np.array_equal(a["position"], i) and np.array_equal(a["subtree"], 70000 - i)
    same(t, ref)
    out = t.select([69000], [69990], None)
    assert out.sum() == 990 and out[69000] == 1 and out[69989] == 1 and out[69990] == 0
    small = t.small_tree((i == 40000).astype(np.uint8))
    assert np.array_equal(small["node_of_vi"], i[:40001]) and np.array_equal(small["parent_vi"], i[:40001] - 1)


@pytest.mark.parametrize("cut", [None] + list(range(taxtree.RANK_NAMES.index("superkingdom"), taxtree.RANK_NAMES.index("strain") + 1)))
def test_select_at_every_cut_rank(cut):
    nodes, ref = reference("random", GENERATED["random"])
    if "random_tree" not in _REF:
        t = device_tree(nodes)
        t.finish()
        _REF["random_tree"] = t
    t = _REF["random_tree"]
    rng = np.random.default_rng(100 + (cut or 0))
    req, exc = rng.choice(ref.n, size=20, replace=False), rng.choice(ref.n, size=5, replace=False)
    want = ref.select(req.tolist(), exc.tolist(), cut)
    got = t.select(req, exc, cut)
    assert np.array_equal(got, want) and t.n_selected == int(want.sum())


@pytest.mark.parametrize("name", sorted(SELECT_CASES))
def test_select_hand_cases(name):
    req, exc, cut, want = SELECT_CASES[name]
    t = device_tree(SELECT_NODES)
    t.finish()
    out = t.select(t.nodes_of(req), t.nodes_of(exc), cut)
    assert t.arrays()["taxids"][out > 0].tolist() == want


def test_select_off_the_root_and_on_a_cycle():
    t = device_tree(CASES["second_self_parent"][0])
    t.finish()
    assert t.arrays()["taxids"][t.select(t.nodes_of([5])) > 0].tolist() == [5, 6]
    t = device_tree(CASES["two_cycle"][0])
    t.finish()
    assert t.arrays()["taxids"][t.select(t.nodes_of([10, 2])) > 0].tolist() == [2, 10]
    for bad in ([8], [9]):
        with pytest.raises(ga.GsError) as e:
            t.select(t.nodes_of(bad))
        assert e.value.code == -1
    with pytest.raises(ga.GsError):
        t.select(t.nodes_of([2]), t.nodes_of([9]))


def test_small_tree_from_host_flags_and_device_regions():
    import torch

    nodes, ref = reference("random", GENERATED["random"])
    t = device_tree(nodes)
    t.finish()
    rng = np.random.default_rng(3)
    for p in (0.0, 0.002, 0.05, 1.0):
        flags = (rng.random(ref.n) < p).astype(np.uint8)
        node_of_vi, parent_vi, depth, position = ref.small_tree(flags)
        regions = torch.from_numpy((flags.astype(np.int32) * rng.integers(1, 9, size=ref.n).astype(np.int32)) - (flags == 0)).to("cuda")
        for f in (flags, regions, torch.from_numpy(flags).to("cuda"), flags.astype(np.int32)):
            got = t.small_tree(f)
            assert np.array_equal(got["node_of_vi"], node_of_vi) and np.array_equal(got["parent_vi"], parent_vi)
            assert np.array_equal(got["depth"], depth) and np.array_equal(got["position"], position)
    b = ga.DeviceDbBuilder(31, len(parent_vi), got["parent_vi"])  # gs_dbbuild_begin takes the tree
    del b
    # a flagged node that the root does not reach stays out
    t = device_tree(CASES["second_self_parent"][0])
    t.finish()
    assert t.small_tree(np.array([0, 1, 0, 1], dtype=np.uint8))["node_of_vi"].tolist() == [0, 1]
    assert t.small_tree(np.array([0, 0, 1, 1], dtype=np.uint8))["node_of_vi"].tolist() == [0]


NAMES_REFUSED = {"one_bar_and_crlf": 0, "negative_name": 1}  # the first line outside the names grammar, 0-based


@pytest.mark.parametrize("name", sorted(NAMES_CASES))
def test_names_cases_on_the_device(name):
    nodes, names, want = NAMES_CASES[name]
    t = device_tree(nodes)
    t.finish()
    rep = t.submit_names(names, last=True)
    lines = names.splitlines(keepends=True)
    if name in NAMES_REFUSED:
        assert rep["refused"] == 1 and rep["taken"] == 0 and rep["first_bad_line"] == NAMES_REFUSED[name], rep
        assert t.names() == [None] * t.n_nodes  # the handle is as it was
        if isinstance(want, tuple):
            with pytest.raises(ga.GsError) as e:
                t.append_names(names, last=True)
            assert e.value.code == -1 and f"line {want[1]}:" in str(e.value)
            return
        t.append_names(names, last=True)
        assert t.names() == want
        return
    assert rep == dict(lines=len(lines), taken=len(lines), refused=0, first_bad_line=-1, longest_line=max(map(len, lines))), rep
    assert t.names() == want
    # every line a chunk of its own: the scientific line in an earlier chunk than a synonym, and in a later one; and the lines
    # by turns on the device and on the host: the line numbers run through both
    for host_turn in (None, 0, 1):
        t = device_tree(nodes)
        t.finish()
        for i, line in enumerate(lines):
            if host_turn is not None and i % 2 == host_turn:
                t.append_names(line, last=i == len(lines) - 1)
            else:
                assert t.submit_names(line, last=i == len(lines) - 1)["refused"] == 0
            if i == 0:
                t.names()  # (a fetch in between changes nothing)
        assert t.names() == want, host_turn


@pytest.mark.parametrize("kind", ["random", "star"])
def test_generated_names_in_one_chunk_and_in_cut_chunks(kind):
    nodes, ref = reference(kind, GENERATED[kind])
    rng = np.random.default_rng(17)
    lines = []
    for t_id in ref.taxids.tolist():
        k = int(rng.integers(0, 4))
        mine = [N(t_id, f"syn {j} of {t_id}") for j in range(k)] + [N(t_id, f"Taxon {t_id} \u00e9", "scientific name")] * int(rng.integers(0, 3))
        if k == 3:
            mine.append(N(t_id, "holds scientific name inside"))
        lines += [mine[i] for i in rng.permutation(len(mine))]
    lines += [N(999999999, "nobody"), N("0x", "nobody"), b"\n", N("007", "nobody")]
    names = b"".join(lines[i] for i in rng.permutation(len(lines)))[:-1]
    want = taxtree.Tree(taxtree.nodes_slots(nodes))
    want.read_names(names)
    assert sum(x is not None for x in want.names) > ref.n // 2
    spots = [4096 * m + d for m in range(1, len(names) // 4096 + 1) for d in (-1, 0, 1)]
    for cuts in ((), cuts_near(names, spots)):
        t = device_tree(nodes)
        t.finish()
        edges = [0] + list(cuts) + [len(names)]
        for a, b in zip(edges, edges[1:]):
            rep = t.submit_names(names[a:b], last=b == len(names))
            assert rep["refused"] == 0 and rep["lines"] == len(names[a:b].splitlines()), (a, b, rep)
        assert t.names() == want.names


def test_names_on_a_tree_that_lives_on_the_host():
    t = device_tree(CASES["dup_same_parent"][0])
    t.finish()
    with pytest.raises(ga.GsError) as e:
        t.submit_names(N(2, "x"), last=True)
    assert e.value.code == -4
    t.append_names(N(2, "x"), last=True)
    assert t.names() == [None, b"x", None]


@pytest.mark.parametrize("name", ["dup_same_parent", "dup_other_parent"])
def test_duplicate_ids_are_reported_and_answered_from_the_host_lists(name):
    nodes, want = CASES[name]
    t = device_tree(nodes)
    info = t.finish()
    assert info["duplicates"] == 1 and info["on_host"] == 1
    ref = taxtree.Tree(taxtree.nodes_slots(nodes))
    same(t, ref)
    assert np.array_equal(t.select([1], [], None), ref.select([1], [], None))
    assert np.array_equal(t.small_tree(np.array([0, 0, 1], dtype=np.uint8))["node_of_vi"], ref.small_tree([0, 0, 1])[0])
    # a larger dump with one line said twice, far apart
    nodes, _ = reference("random", GENERATED["random"])
    lines = nodes.splitlines(keepends=True)
    nodes = b"".join(lines + [lines[1234]])
    t = device_tree(nodes)
    assert t.finish()["duplicates"] == 1
    same(t, taxtree.Tree(taxtree.nodes_slots(nodes)))


def test_call_order_and_arguments():
    t = ga.DeviceTaxTree()
    for call in (t.arrays, t.names, lambda: t.select([0]), lambda: t.small_tree(np.zeros(0, dtype=np.uint8)), lambda: t.submit_names(b"1\t|\tx\t|\n"), lambda: t.append_names(b"1\t|\tx\t|\n"), t.finish_times):
        with pytest.raises(ga.GsError) as e:
            call()
        assert e.value.code == -5
    with pytest.raises(ga.GsError) as e:
        t.finish()
    assert e.value.code == -1  # no line at all: no root
    t.submit_nodes(CASES["golden"][0], last=True)
    t.finish()
    for call in (t.finish, lambda: t.submit_nodes(b"\n"), lambda: t.append_nodes(b"\n")):
        with pytest.raises(ga.GsError) as e:
            call()
        assert e.value.code == -5
    with pytest.raises(ga.GsError) as e:
        t.select([3])
    assert e.value.code == -1
    n, ms = t.kernel_time()
    assert n == 0 and ms == 0
    t.select([0])
    n, ms = t.kernel_time()
    assert n == 1 and ms > 0
