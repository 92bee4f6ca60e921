"""The taxtree and taxnodes goals without a GPU: the plain-Python restatement (tests/taxtree.py) against the hand-worked cases, and
gs_taxparse.h under the host-only handle (device -1) against the restatement, on the cases and on generated dumps."""
import ctypes as C

import numpy as np
import pytest

import genestrip_amd as ga
import taxtree
from taxtree_cases import (CASES, FIRST_BAD, IN_GRAMMAR, NAMES_CASES, SELECT_CASES, SELECT_NODES, TAXIDS_EXPECT, TAXIDS_NUMBERS, TAXIDS_TEXT,
                           chain_dump, random_dump, star_dump)

KEYS = ("taxids", "parent", "depth", "position", "subtree", "rank")


def reference(nodes):
    return taxtree.Tree(taxtree.nodes_slots(nodes))


def ref_arrays(t):
    return {k: getattr(t, k) for k in KEYS}


def host_tree(nodes, names=None, pieces=1):
    t = ga.DeviceTaxTree(device=-1)
    cuts = [0] + [nodes.rfind(b"\n", 0, len(nodes) * i // pieces) + 1 for i in range(1, pieces)] + [len(nodes)]
    for a, b in zip(cuts, cuts[1:]):
        t.append_nodes(nodes[a:b], last=b == len(nodes))
    t.finish()
    if names is not None:
        t.append_names(names, last=True)
    return t


def same(got, want):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (k, got[k][:20], want[k][:20])


# (this test and test_grammar_predicate_sorts_the_cases check the oracle itself -- tests/taxtree.py against the values worked by hand
# -- and touch no symbol of the library: they would pass without it.  Everything else in this file goes through the C ABI.)
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_hand_worked_arrays(name):
    nodes, want = CASES[name]
    if isinstance(want, tuple):
        with pytest.raises(taxtree.Throws if want[0] == "throws" else taxtree.Unsupported) as e:
            reference(nodes)
        assert e.value.line == want[1]
        return
    same(ref_arrays(reference(nodes)), want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_only_handle_gives_the_hand_worked_arrays(name):
    nodes, want = CASES[name]
    if isinstance(want, tuple):
        with pytest.raises(ga.GsError) as e:
            host_tree(nodes)
        assert e.value.code == (-1 if want[0] == "throws" else -4)
        if want[1]:
            assert f"line {want[1]}:" in str(e.value)
        return
    t = host_tree(nodes)
    same(t.arrays(), want)
    assert t.on_host == 1 and t.n_duplicates == reference(nodes).duplicates


def test_grammar_predicate_sorts_the_cases():
    for name, (nodes, _) in CASES.items():
        lines = nodes.splitlines(keepends=True)
        bad = [i for i, line in enumerate(lines) if not taxtree.in_nodes_grammar(line)]
        assert (bad[0] if bad else None) == FIRST_BAD.get(name), name
        assert (name in IN_GRAMMAR) == (not bad), name


def test_a_failed_append_leaves_the_handle_as_it_was():
    t = ga.DeviceTaxTree(device=-1)
    good = CASES["golden"][0]
    t.append_nodes(good[:good.index(b"\n") + 1])
    with pytest.raises(ga.GsError) as e:
        t.append_nodes(b"2a\t|\t1\t|\tno rank\t|\n")
    assert "line 2:" in str(e.value)
    t.append_nodes(good[good.index(b"\n") + 1:], last=True)
    t.finish()
    same(t.arrays(), CASES["golden"][1])


@pytest.mark.parametrize("name", sorted(NAMES_CASES))
def test_names(name):
    nodes, names, want = NAMES_CASES[name]
    ref = reference(nodes)
    if isinstance(want, tuple):
        with pytest.raises(taxtree.Throws) as e:
            ref.read_names(names)
        assert e.value.line == want[1]
        with pytest.raises(ga.GsError) as e:
            host_tree(nodes, names)
        assert e.value.code == -1 and f"line {want[1]}:" in str(e.value)
        return
    ref.read_names(names)
    assert ref.names == want
    assert host_tree(nodes, names).names() == want


def test_taxids_file():
    assert taxtree.read_taxids(TAXIDS_TEXT) == TAXIDS_EXPECT
    req, exc = ga.read_taxids(TAXIDS_TEXT)
    assert (req.tolist(), exc.tolist()) == TAXIDS_NUMBERS
    ref = reference(SELECT_NODES)
    assert taxtree.taxid_nodes(ref, ["4", "007", "12x", "", "99", "12"]) == [ref.node_of(4), ref.node_of(12)]


@pytest.mark.parametrize("name", sorted(SELECT_CASES))
def test_selection(name):
    req, exc, cut, want = SELECT_CASES[name]
    ref = reference(SELECT_NODES)
    cut_o = None if cut is None else taxtree.RANK_NAMES.index(cut)
    nodes = lambda ids: [ref.node_of(i) for i in ids if ref.node_of(i) >= 0]
    got = ref.select(nodes(req), nodes(exc), cut_o)
    assert ref.taxids[got > 0].tolist() == want
    t = host_tree(SELECT_NODES)
    out = t.select(t.nodes_of(req), t.nodes_of(exc), cut)
    assert np.array_equal(out, got) and t.n_selected == len(want)


def test_selection_descends_what_the_root_does_not_reach_and_fails_on_a_cycle():
    nodes = CASES["second_self_parent"][0]
    ref, t = reference(nodes), host_tree(nodes)
    want = ref.select([ref.node_of(5)], [], None)
    assert ref.taxids[want > 0].tolist() == [5, 6] and np.array_equal(t.select(t.nodes_of([5])), want)
    nodes = CASES["two_cycle"][0]
    ref, t = reference(nodes), host_tree(nodes)
    assert ref.taxids[ref.select([ref.node_of(10)], [], None) > 0].tolist() == [10]
    assert np.array_equal(t.select(t.nodes_of([10])), ref.select([ref.node_of(10)], [], None))
    with pytest.raises(taxtree.Throws):
        ref.select([ref.node_of(8)], [], None)
    with pytest.raises(ga.GsError):
        t.select(t.nodes_of([8]))


def _small_same(t, ref, flags):
    got = t.small_tree(flags)
    node_of_vi, parent_vi, depth, position = ref.small_tree(flags)
    assert np.array_equal(got["node_of_vi"], node_of_vi) and np.array_equal(got["parent_vi"], parent_vi)
    assert np.array_equal(got["depth"], depth) and np.array_equal(got["position"], position)
    return got


def test_small_tree_hand_cases():
    ref, t = reference(SELECT_NODES), host_tree(SELECT_NODES)
    flags = np.zeros(ref.n, dtype=np.uint8)
    flags[[ref.node_of(8), ref.node_of(12)]] = 1  # two leaves under the shared ancestor 6
    got = _small_same(t, ref, flags)
    assert ref.taxids[got["node_of_vi"]].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 12]
    assert got["parent_vi"].tolist() == [-1, 0, 1, 2, 3, 4, 5, 6, 5] and got["position"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9]
    # without a flag the root alone; int32 counts read as flags; a flagged node the root does not reach stays out
    assert _small_same(t, ref, np.zeros(ref.n, dtype=np.uint8))["node_of_vi"].tolist() == [0]
    _small_same(t, ref, (flags * 7).astype(np.int32) - 1 + (flags > 0))
    nodes = CASES["second_self_parent"][0]
    ref, t = reference(nodes), host_tree(nodes)
    flags = np.zeros(ref.n, dtype=np.uint8)
    flags[[ref.node_of(6), ref.node_of(2)]] = 1
    assert ref.taxids[_small_same(t, ref, flags)["node_of_vi"]].tolist() == [1, 2]


GENERATED = {"random": lambda: random_dump(5000, seed=11), "chain": lambda: chain_dump(3000), "star": lambda: star_dump(10000)}


@pytest.mark.parametrize("kind", sorted(GENERATED))
def test_generated_dumps(kind):
    nodes = GENERATED[kind]()
    ref = reference(nodes)
    t = host_tree(nodes, pieces=7)
    same(t.arrays(), ref_arrays(ref))
    assert t.n_reached == ref.n and t.max_depth == int(ref.depth.max())
    if kind == "chain":
        assert t.max_depth == 2999 and ref.subtree[0] == 3000
    rng = np.random.default_rng(5)
    for cut in (None, "species", "genus"):
        req, exc = rng.choice(ref.n, size=12, replace=False), rng.choice(ref.n, size=4, replace=False)
        want = ref.select(req.tolist(), exc.tolist(), None if cut is None else taxtree.RANK_NAMES.index(cut))
        assert np.array_equal(t.select(req, exc, cut), want)
    _small_same(t, ref, (rng.random(ref.n) < 0.01).astype(np.uint8))


def test_arguments_and_call_order():
    """(there is no device on this machine: a call that reached one would answer -6)"""
    L = ga.lib()
    h = C.c_void_p()
    rep = (C.c_int64 * 8)()
    assert L.gs_taxtree_create(None, -1) == -1 and L.gs_taxtree_create(C.byref(h), -2) == -1
    assert L.gs_taxtree_submit_nodes(None, None, 0, 0, 0, rep) == -1 and L.gs_taxtree_finish_nodes(None, rep) == -1
    assert L.gs_taxtree_create(C.byref(h), -1) == 0
    text = np.frombuffer(CASES["golden"][0], dtype=np.uint8)
    p = text.ctypes.data_as(C.c_void_p)
    assert L.gs_taxtree_submit_nodes(h, p, len(text), 0, 1, rep) == -4  # host only
    assert L.gs_taxtree_append_nodes(h, p, -1, 1, rep) == -1 and L.gs_taxtree_append_nodes(h, None, 5, 1, rep) == -1
    out = np.zeros(8, dtype=np.int32)
    o = out.ctypes.data_as(C.c_void_p)
    assert L.gs_taxtree_fetch(h, o, None, None, None, None, None) == -5 and L.gs_taxtree_append_names(h, p, 0, 1) == -5
    assert L.gs_taxtree_submit_names(h, p, len(text), 0, 1, rep) == -5 and L.gs_taxtree_finish_times(h, rep) == -5
    assert L.gs_taxtree_select(h, None, 0, None, 0, -1, o, None) == -5 and L.gs_taxtree_small(h, o, 1, 0, o, None, None, None, None) == -5
    assert L.gs_taxtree_append_nodes(h, p, len(text), 1, rep) == 0 and rep[0] == 3 and rep[2] == 3
    assert L.gs_taxtree_finish_nodes(h, rep) == 0 and rep[0] == 3 and rep[1] == 3 and rep[4] == 1
    assert L.gs_taxtree_finish_nodes(h, rep) == -5 and L.gs_taxtree_append_nodes(h, p, len(text), 1, rep) == -5
    assert L.gs_taxtree_submit_names(h, p, len(text), 0, 1, rep) == -4 and L.gs_taxtree_submit_names(h, p, -1, 0, 1, rep) == -1  # the tree lives on the host
    ms = (C.c_double * 3)()
    assert L.gs_taxtree_finish_times(h, ms) == 0 and tuple(ms) == (0.0, 0.0, 0.0) and L.gs_taxtree_finish_times(h, None) == -1
    assert L.gs_taxtree_select(h, o, -1, None, 0, -1, o, None) == -1 and L.gs_taxtree_select(h, None, 0, None, 0, 40, o, None) == -1
    out[0] = 3
    assert L.gs_taxtree_select(h, o, 1, None, 0, -1, o, None) == -1  # no node 3
    assert L.gs_taxtree_small(h, o, 2, 0, o, None, None, None, None) == -1 and L.gs_taxtree_small(h, o, 1, 1, o, None, None, None, None) == -4
    assert L.gs_taxtree_destroy(h) == 0 and L.gs_taxtree_destroy(None) == 0


# ---- the host layer without a device (GS_HOST_FAST=0): gs_host_taxtree_files through gs_taxparse.h into a host-only tree
import gzip  # noqa: E402

from conftest import bgzf  # noqa: E402
from genestrip_amd import host  # noqa: E402
from taxtree_cases import NAMES_NODES, N  # noqa: E402


@pytest.mark.parametrize("container", ["plain", "gz", "bgzf"])
def test_host_layer_on_files(container, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    pack = {"plain": lambda d: d, "gz": gzip.compress, "bgzf": lambda d: bgzf(d, block=4000)}[container]
    ext = "" if container == "plain" else ".gz"
    lines = random_dump(4000, seed=21).splitlines(keepends=True)
    # oddities between the lines: a line the reference skips, an empty one, CRLF, a line beyond the buffer; no final newline
    odd = [b"77\t|\n", b"\n", lines[5][:-1] + b"\r\n", lines[6][:-1] + b"x" * 5000 + b"\n"]
    nodes = b"".join(ln + (odd[(i // 97) % 4] if i % 97 == 0 and i > 6 else b"") for i, ln in enumerate(lines))[:-1]
    ref = reference(nodes)
    names = b"".join(N(int(t), f"name {t}", "scientific name" if t % 3 else "synonym") for t in ref.taxids[::-1]) + N(1, "late synonym")
    ref.read_names(names)
    (tmp_path / ("nodes.dmp" + ext)).write_bytes(pack(nodes))
    (tmp_path / ("names.dmp" + ext)).write_bytes(pack(names))
    t, rep = host.taxtree_files(tmp_path / ("nodes.dmp" + ext), tmp_path / ("names.dmp" + ext))
    assert t.device == -1 and rep["device_chunks"] == 0 and rep["on_host"] == 1 and rep["nodes"] == ref.n and rep["reached"] == ref.n
    assert rep["nodes_lines"] == len(taxtree.next_lines(nodes)) and rep["names_lines"] == ref.n + 1 and rep["duplicates"] == ref.duplicates > 0
    same(t.arrays(), ref_arrays(ref))
    assert t.names() == ref.names
    t2, rep2 = host.taxtree_files(tmp_path / ("nodes.dmp" + ext))
    assert t2.names() == [None] * ref.n and rep2["names_lines"] == 0


def test_host_layer_names_the_file_and_the_line(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    path = tmp_path / "nodes.dmp"
    path.write_bytes(CASES["no_digit"][0])
    with pytest.raises(ga.GsError) as e:
        host.taxtree_files(path)
    assert e.value.code == -1 and str(path) in str(e.value) and "line 3:" in str(e.value)
    path.write_bytes(CASES["no_root"][0])
    with pytest.raises(ga.GsError) as e:
        host.taxtree_files(path)
    assert e.value.code == -1 and "no root" in str(e.value)
    with pytest.raises(ga.GsError) as e:
        host.taxtree_files(tmp_path / "missing.dmp")
    assert e.value.code == -7


def test_taxids_file_through_the_host_layer(tmp_path):
    path = tmp_path / "taxids.txt"
    path.write_bytes(TAXIDS_TEXT)
    req, exc = host.read_taxids_file(path)
    assert (req.tolist(), exc.tolist()) == TAXIDS_NUMBERS
    gz = tmp_path / "taxids.txt.gz"
    gz.write_bytes(gzip.compress(TAXIDS_TEXT))
    req, exc = host.read_taxids_file(gz)
    assert (req.tolist(), exc.tolist()) == TAXIDS_NUMBERS
