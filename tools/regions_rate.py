#!/usr/bin/env python3
"""Rates of gs_taxtree_regions_below on a generated tree of NCBI's shape.

    python tools/regions_rate.py [nodes]        (default 2 600 000)

The tree: the parent of node i drawn uniformly among the nodes in front of it; regions: one node in twenty carries 1-40 entries; the
selection: every node; the limit 10, the rank species.  Five turns after one untimed, the two ways by turns, fastest and slowest:
  device tree, between events (kernel_time): the counts (scatter, scan, difference) and the selection (mark, flag, scan, compaction)
  device tree, host clock around the call: regions in device memory, and in host memory
  host-only tree (device -1), host clock around the call: the parent walk per node with entries"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402

RANKS = ["no rank", "species", "genus", "strain", "clade", "family", "subspecies", "order", "class", "phylum", "superkingdom"]


def ncbi_shaped(n, seed=1):
    rng = np.random.default_rng(seed)
    ids = np.cumsum(rng.integers(1, 4, size=n)).astype(np.int64)
    ids[0] = 1
    ids[1:] += 1
    parent = np.zeros(n, dtype=np.int64)
    parent[1:] = (np.arange(1, n) * rng.random(n - 1)).astype(np.int64)
    pick = rng.integers(0, len(RANKS), size=n).tolist()
    ids, parent = ids.tolist(), parent.tolist()
    return "".join(f"{ids[k]}\t|\t{ids[parent[k]]}\t|\t{RANKS[pick[k]]}\t|\n" for k in range(n)).encode()


def spread(times, unit="ms"):
    return f"{min(times):.3f} {unit} ({max(times):.3f})"


def main():
    import torch

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_600_000
    t0 = time.perf_counter()
    nodes = ncbi_shaped(n)
    print(f"generated {n} nodes ({len(nodes) / 1e6:.1f} MB) in {time.perf_counter() - t0:.1f} s", flush=True)
    dev = ga.DeviceTaxTree()
    assert dev.submit_nodes(torch.from_numpy(np.frombuffer(nodes, dtype=np.uint8).copy()).to("cuda"), last=True)["refused"] == 0
    info = dev.finish()
    t0 = time.perf_counter()
    hst = ga.DeviceTaxTree(device=-1)
    hst.append_nodes(nodes, last=True)
    hst.finish()
    print(f"tree: {info['nodes']} nodes, {info['reached']} reached, deepest at {info['max_depth']}; the host-only tree took {time.perf_counter() - t0:.1f} s", flush=True)
    rng = np.random.default_rng(2)
    regions = np.where(rng.random(n) < 0.05, rng.integers(1, 41, n), 0).astype(np.int32)
    regions_dev = torch.from_numpy(regions).to("cuda")
    selected = np.arange(n, dtype=np.int32)
    events, wall_dev, wall_host_mem, wall_host = [], [], [], []
    dev.kernel_time(True)
    for turn in range(6):
        ms0 = dev.kernel_time()[1]
        t0 = time.perf_counter()
        below_d, incl_d = dev.regions_below(regions_dev, selected, 10, "species")
        t1 = time.perf_counter()
        ms1 = dev.kernel_time()[1]
        t2 = time.perf_counter()
        dev.regions_below(regions, selected, 10, "species")
        t3 = time.perf_counter()
        below_h, incl_h = hst.regions_below(regions, selected, 10, "species")
        t4 = time.perf_counter()
        assert np.array_equal(below_d, below_h) and np.array_equal(incl_d, incl_h)
        if turn:
            events.append(ms1 - ms0)
            wall_dev.append((t1 - t0) * 1e3)
            wall_host_mem.append((t3 - t2) * 1e3)
            wall_host.append((t4 - t3) * 1e3)
    print(f"  {int(regions.sum())} entries at {int((regions > 0).sum())} nodes; {len(below_d)} of {n} selected nodes are species below 10")
    print(f"  device tree, kernels between events (counts + selection)      {spread(events)}")
    print(f"  device tree, the call, regions in device memory                {spread(wall_dev)}")
    print(f"  device tree, the call, regions in host memory                  {spread(wall_host_mem)}")
    print(f"  host-only tree, the call (parent walk per node with entries)   {spread(wall_host)}")
    dev.close()
    hst.close()


if __name__ == "__main__":
    main()
