"""host.taxtree_files (gs_host_taxtree_files: NCBI dump files -> the tree, nodes chunks on the device, what it refuses through
gs_taxparse.h) against the plain-Python restatement (tests/taxtree.py) and against the same call under GS_HOST_FAST=0, and the road
from a dump to a store.  Needs an MI355X: run with -m gpu."""
import gzip

import numpy as np
import pytest

import accmap
import genestrip_amd as ga
import taxtree
from accmap_cases import CFG
from accmap_cases import L as CL
from conftest import bgzf
from genestrip_amd import host
from progresscheck import check_records, run
from taxtree_cases import CASES, L, N, random_dump

pytestmark = pytest.mark.gpu

SMALLEST_BLOCK = 64  # reader_shape() of gs_host.cpp takes GS_HOST_BLOCK_BYTES from 64 on
KEYS = ("taxids", "parent", "depth", "position", "subtree", "rank")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _pack(container, data):
    return data if container == "plain" else gzip.compress(data, 6) if container == "gz" else bgzf(data, block=3000)


def _same(t, ref):
    got = t.arrays()
    for k in KEYS:
        assert np.array_equal(got[k], getattr(ref, k)), (k, got[k][:16], getattr(ref, k)[:16])


@pytest.mark.parametrize("container", ["plain", "gz", "bgzf"])
@pytest.mark.parametrize("block", [SMALLEST_BLOCK, 4096])
def test_dump_files_on_the_device_and_line_by_line(container, block, tmp_path, monkeypatch):
    """chunk cuts inside the dump; lines outside the device's grammar between chunks that the device takes; no final newline"""
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", str(block))
    lines = random_dump(1200 if block == SMALLEST_BLOCK else 5000, seed=31, max_id=90000).splitlines(keepends=True)
    # (an inflated file of this size reaches the cutter as one block: with an odd line in it the device would take none of it)
    odd = lambda j: [b"77\t|\n", b"9\x00%04d\t|\t1\t|\tgenus\t|\n" % j, b"9%04d\t|\t1\t|\n" % (5000 + j), b"\n"][j % 4] if container == "plain" else b""
    every = len(lines) // 9
    nodes = b"".join(ln + (odd(i // every) if i % every == 0 and i else b"") for i, ln in enumerate(lines))[:-1]
    ref = taxtree.Tree(taxtree.nodes_slots(nodes))
    names = b"".join(N(int(t), f"n{t}", "scientific name" if t % 2 else "synonym") for t in ref.taxids) + N(1, "a synonym of the root")
    ref.read_names(names)
    ext = "" if container == "plain" else ".gz"
    p_nodes, p_names = tmp_path / ("nodes.dmp" + ext), tmp_path / ("names.dmp" + ext)
    p_nodes.write_bytes(_pack(container, nodes))
    p_names.write_bytes(_pack(container, names))
    t, rep = host.taxtree_files(p_nodes, p_names)
    assert t.device == 0 and rep["device_chunks"] > 0 and rep["host_chunks"] > 0 and rep["on_host"] == 0, rep
    assert (rep["nodes"], rep["reached"], rep["duplicates"], rep["nodes_lines"]) == (ref.n, int((ref.position >= 0).sum()), 0, len(taxtree.next_lines(nodes)))
    _same(t, ref)
    assert t.names() == ref.names
    monkeypatch.setenv("GS_HOST_FAST", "0")
    th, reph = host.taxtree_files(p_nodes, p_names)
    assert th.device == -1 and reph["device_chunks"] == 0 and reph["on_host"] == 1
    assert {k: reph[k] for k in ("nodes", "reached", "duplicates", "nodes_lines", "names_lines")} == {k: rep[k] for k in ("nodes", "reached", "duplicates", "nodes_lines", "names_lines")}
    _same(th, ref)
    assert th.names() == ref.names


def test_a_line_beyond_a_block_sends_the_rest_line_by_line(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "4096")
    lines = random_dump(3000, seed=33).splitlines(keepends=True)
    nodes = b"".join(lines[:1500]) + lines[1500][:-1] + b"x" * 5000 + b"\n" + b"".join(lines[1501:])
    ref = taxtree.Tree(taxtree.nodes_slots(nodes))
    path = tmp_path / "nodes.dmp"
    path.write_bytes(nodes)
    t, rep = host.taxtree_files(path)
    assert rep["device_chunks"] > 3 and rep["host_chunks"] >= 1 and rep["nodes_lines"] == 3001  # (the long line is two: its rest holds no bar and is skipped)
    _same(t, ref)
    # a bad line fails with the file and its line, whichever way its chunk went
    path.write_bytes(b"".join(lines[:2000]) + L("2a", 1) + b"".join(lines[2000:]))
    with pytest.raises(ga.GsError) as e:
        host.taxtree_files(path)
    assert e.value.code == -1 and str(path) in str(e.value) and "line 2001:" in str(e.value)


def test_progress_records_and_cancellation(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "4096")
    nodes = random_dump(3000, seed=35)
    p = tmp_path / "nodes.dmp"
    p.write_bytes(nodes)
    paths = [str(p)]
    call = lambda: host.taxtree_files(paths[0])
    (t, rep), stop, records = run(call)
    assert stop is None and rep["nodes_lines"] == 3000 and rep["device_chunks"] > 10
    assert check_records(records, paths, complete=True)[0] == 3000
    got, stop, recs = run(call, stop_at=2)  # behind the first chunk
    k = check_records(recs, paths, complete=False)[0]
    assert got is None and stop.code == -8 and 0 < k < 3000


def test_from_a_dump_to_a_store(tmp_path):
    """dump -> tree -> taxnodes -> accession map over the tree's ids -> regions -> small tree -> build: the store of the same build
    driven by arrays made by hand (the restatement's small tree)"""
    nodes = random_dump(600, seed=37, max_id=5000)
    (tmp_path / "nodes.dmp").write_bytes(nodes)
    (tmp_path / "taxids.txt").write_bytes(b"# the whole tree but one branch\n1\n")
    t, rep = host.taxtree_files(tmp_path / "nodes.dmp")
    ref = taxtree.Tree(taxtree.nodes_slots(nodes))
    a = t.arrays()
    req, exc = host.read_taxids_file(tmp_path / "taxids.txt")
    branch = int(np.flatnonzero((ref.subtree > 5) & (ref.subtree < 60))[0])
    selected = t.select(t.nodes_of(req), [branch], "species")
    assert np.array_equal(selected, ref.select([0], [branch], taxtree.RANK_NAMES.index("species"))) and 10 < selected.sum() < ref.n
    # a catalog that names every fourth selected node, and some that are not selected
    picked = np.flatnonzero(selected)[::4]
    catalog = b"".join(CL(str(int(a["taxids"][v])), f"NC_{i:06d}.1") for i, v in enumerate(list(picked) + [branch]))
    m = ga.DeviceAccessionMap(a["taxids"], CFG["categories"], CFG["statuses"], CFG["seq_type"])
    assert m.submit(catalog, last=True)["refused"] == 0
    m.finish()
    slots, entry_nodes, regions = m.fetch()
    assert regions.sum() == len(picked) + 1
    flagged = np.where(selected > 0, regions, 0).astype(np.int32)
    small = t.small_tree(flagged)
    want = ref.small_tree(flagged)
    assert np.array_equal(small["node_of_vi"], want[0]) and np.array_equal(small["parent_vi"], want[1]) and len(want[0]) > len(picked)
    vi_of_node = np.full(ref.n, -1, dtype=np.int32)
    vi_of_node[small["node_of_vi"]] = np.arange(len(small["node_of_vi"]), dtype=np.int32)
    rng = np.random.default_rng(39)
    genomes = [ACGT[rng.integers(0, 4, 400)] for _ in picked]
    seq = np.concatenate(genomes)
    off = np.concatenate([[0], np.cumsum([len(g) for g in genomes])]).astype(np.uint64)

    def build(parent_vi, node_vi):
        b = ga.DeviceDbBuilder(31, len(parent_vi), parent_vi)
        for u in (False, True):
            b.add(seq, off, node_vi, update=u)
        out = b.finish()
        b.close()
        return out

    got = build(small["parent_vi"], vi_of_node[picked])
    by_hand_vi = {int(n): i for i, n in enumerate(want[0])}
    hand = build(want[1], np.array([by_hand_vi[int(v)] for v in picked], dtype=np.int32))
    assert np.array_equal(got[0], hand[0]) and np.array_equal(got[1], hand[1]) and len(got[0]) > 1000
