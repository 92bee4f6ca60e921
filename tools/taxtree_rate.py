#!/usr/bin/env python3
"""Rates of the tree handle (gs_taxtree) on a generated dump of NCBI's shape, and on a chain.

    python tools/taxtree_rate.py [nodes]        (default 2 600 000)

Between events (kernel_time of the handles), fastest and slowest of five turns after one untimed: the nodes scan of the whole dump as
one chunk resident on the device, the finish and its three phases (distinct ids and parents: a key sort, a scan, the searches; child
order: a pair sort; tree steps: Euler tour, pointer jumping, cycles), a select, a small tree and the names scan of the whole
names text as one chunk; as yardsticks gs_accmap's count pass and the four-line text stage of gs_reads on the nodes bytes.  A second row: a chain of 1 000 000 nodes, as deep as it has nodes.  End to end, host clock, three turns
each by turns: host.taxtree_files from a plain and a .gz file, device path and GS_HOST_FAST=0."""
import ctypes as C
import gzip
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host  # noqa: E402

RANKS = ["no rank", "species", "genus", "strain", "clade", "family", "subspecies", "order", "class", "phylum", "superkingdom"]


def ncbi_shaped(n, seed=1):
    """n nodes: the parent of node i is drawn uniformly among the nodes in front of it, which puts the deepest
    node near depth 40; ids ascend with gaps; lines in id order, as NCBI writes them -> (nodes bytes, names bytes, max depth)"""
    rng = np.random.default_rng(seed)
    ids = np.cumsum(rng.integers(1, 4, size=n)).astype(np.int64)
    ids[0] = 1
    ids[1:] += 1
    parent = np.zeros(n, dtype=np.int64)
    i = np.arange(1, n)
    parent[1:] = (i * rng.random(n - 1)).astype(np.int64)  # (uniform attachment: the deepest node lies near e ln n)
    ids, parent = ids.tolist(), parent.tolist()
    depth = [0] * n
    for k in range(1, n):  # (a Python loop: some seconds for 2.6 M)
        depth[k] = depth[parent[k]] + 1
    pick = rng.integers(0, len(RANKS), size=n).tolist()
    tail = "\t|\t\t|\t8\t|\t0\t|\t1\t|\t0\t|\t0\t|\t0\t|\t0\t|\t0\t|\t\t|\n"
    nodes = "".join(f"{ids[k]}\t|\t{ids[parent[k]]}\t|\t{RANKS[pick[k]]}{tail}" for k in range(n)).encode()
    syn = (rng.random(n) < 0.5).tolist()
    names = "".join(f"{ids[k]}\t|\tTaxon {ids[k]}\t|\t\t|\tscientific name\t|\n" + (f"{ids[k]}\t|\told name {k}\t|\t\t|\tsynonym\t|\n" if syn[k] else "")
                    for k in range(n)).encode()
    return nodes, names, max(depth)


def chain(n):
    return "1\t|\t1\t|\tno rank\t|\n".encode() + "".join(f"{k}\t|\t{k - 1}\t|\tspecies\t|\n" for k in range(2, n + 1)).encode()


def spread(times):
    return f"{min(times):.3f} ms ({max(times):.3f})"


def device_rows(label, nodes, names=None, turns=5):
    import torch

    text = torch.from_numpy(np.frombuffer(nodes, dtype=np.uint8).copy()).to("cuda")
    scan, finish, select, small, phases, nscan = [], [], [], [], [], []
    names_dev = None if names is None else torch.from_numpy(np.frombuffer(names, dtype=np.uint8).copy()).to("cuda")
    info = None
    for turn in range(turns + 1):
        t = ga.DeviceTaxTree()
        t.kernel_time(True)
        rep = t.submit_nodes(text, last=True)
        assert rep["refused"] == 0, rep
        ms0 = t.kernel_time()[1]
        info = t.finish()
        ms1 = t.kernel_time()[1]
        rng = np.random.default_rng(turn)
        req = rng.choice(info["nodes"], size=100, replace=False)
        out = t.select(req, (req[:5] + 1) % info["nodes"], "species")
        ms2 = t.kernel_time()[1]
        sm = t.small_tree((rng.random(info["nodes"]) < 0.01).astype(np.uint8))
        ms3 = t.kernel_time()[1]
        if names_dev is not None:
            assert t.submit_names(names_dev, last=True)["refused"] == 0
        ms4 = t.kernel_time()[1]
        if turn:
            phases.append(t.finish_times())
            nscan.append(ms4 - ms3)
            scan.append(ms0)
            finish.append(ms1 - ms0)
            select.append(ms2 - ms1)
            small.append(ms3 - ms2)
        n_sel, n_small = int(out.sum()), len(sm["node_of_vi"])
        t.close()
    mb = len(nodes) / 1e6
    print(f"{label}: {info['nodes']} nodes, {mb:.1f} MB, max depth {info['max_depth']}")
    print(f"  nodes scan        {spread(scan)}  = {mb / min(scan):.1f} GB/s of text")
    print(f"  finish            {spread(finish)}")
    for i, what in enumerate(("distinct ids and parents (key sort, scan, searches)", "child order (pair sort, links)", "tree steps (Euler tour, jumping, cycles)")):
        print(f"    {what}  {spread([p[i] for p in phases])}")
    print(f"  select (100 requested, 5 excluded, cut species: {n_sel} in)  {spread(select)}  (with the copy of the flags to the host)")
    print(f"  small tree (1 % flagged: {n_small} values)  {spread(small)}  (with the copies of the flags in and the arrays out)")
    if names_dev is not None:
        print(f"  names scan ({len(names) / 1e6:.1f} MB: tiles, grammar, votes, gather)  {spread(nscan)}  = {len(names) / 1e6 / min(nscan):.1f} GB/s of text")
    return text


def accmap_yardstick(text, turns=5):
    m = ga.DeviceAccessionMap(np.array([1], dtype=np.int32), ["x"], ["x"])
    m.kernel_time(True)
    times, before = [], 0.0
    for turn in range(turns + 1):
        m.submit(text, last=True)
        now = m.kernel_time()[1]
        if turn:
            times.append(now - before)
        before = now
    m.close()
    print(f"  yardstick: gs_accmap count pass on the same bytes (refused)  {spread(times)}")


def text_stage_yardstick(text, nodes, turns=5):
    """the four-line text stage of gs_reads on the same bytes, as tools/accmap_rate.py runs it"""
    import torch

    n = nodes.count(b"\n")
    reads = ga.DeviceReads(k=31)
    L = ga.lib()
    acc = torch.zeros(max(n // 4, 1), dtype=torch.uint8, device="cuda:0")
    key = np.frombuffer(b"x", dtype=np.uint8)
    nl = n & ~3
    cut = len(nodes) if nl == n else int(np.flatnonzero(np.frombuffer(nodes, dtype=np.uint8) == 10)[nl - 1]) + 1
    reads.kernel_time(True)
    times = []
    for turn in range(turns + 1):
        before = reads.phase_times()["select"][1]
        L.gs_reads_select_text(reads.h, 31, C.c_void_p(text.data_ptr()), cut, nl, ga.MEM_DEVICE, key.ctypes.data_as(C.c_void_p), 1, C.c_void_p(acc.data_ptr()), None, None)
        L.gs_reads_sync(reads.h)
        reads.text_reset(True)
        if turn:
            times.append(reads.phase_times()["select"][1] - before)
    reads.close()
    print(f"  yardstick: gs_reads four-line text stage on the same bytes (refused)  {spread(times)}  = {cut / 1e6 / min(times):.1f} GB/s")


def end_to_end(nodes, names, turns=3):
    with tempfile.TemporaryDirectory() as d:
        files = {}
        for kind in ("plain", "gz"):
            ext = "" if kind == "plain" else ".gz"
            files[kind] = (os.path.join(d, "nodes.dmp" + ext), os.path.join(d, "names.dmp" + ext))
            for path, data in zip(files[kind], (nodes, names)):
                with open(path, "wb") as f:
                    f.write(data if kind == "plain" else gzip.compress(data, 1))
        for kind in ("plain", "gz"):
            for with_names in (False, True):
                res = {"device": [], "host": []}
                for turn in range(turns):
                    for way in ("device", "host"):
                        os.environ["GS_HOST_FAST"] = "1" if way == "device" else "0"
                        t0 = time.perf_counter()
                        t, rep = host.taxtree_files(files[kind][0], files[kind][1] if with_names else None)
                        res[way].append(time.perf_counter() - t0)
                        if way == "device":
                            chunks = (rep["device_chunks"], rep["host_chunks"])
                        t.close()
                os.environ.pop("GS_HOST_FAST", None)
                print(f"  taxtree_files {kind:5s} {'nodes + names' if with_names else 'nodes alone  '}: device path {min(res['device']):.3f} s ({max(res['device']):.3f})"
                      f"   GS_HOST_FAST=0 {min(res['host']):.3f} s ({max(res['host']):.3f})   device path: {chunks[0]} device and {chunks[1]} host chunks")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_600_000
    t0 = time.perf_counter()
    nodes, names, deepest = ncbi_shaped(n)
    print(f"generated {n} nodes ({len(nodes) / 1e6:.1f} MB) and names ({len(names) / 1e6:.1f} MB) in {time.perf_counter() - t0:.1f} s; max depth {deepest}", flush=True)
    text = device_rows("NCBI-shaped", nodes, names)
    accmap_yardstick(text)
    text_stage_yardstick(text, nodes)
    del text
    sys.stdout.flush()
    device_rows("chain", chain(min(n, 1_000_000)))
    sys.stdout.flush()
    end_to_end(nodes, names)


if __name__ == "__main__":
    main()
