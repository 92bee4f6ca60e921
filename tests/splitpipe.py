"""The DB-partitioned pipeline encode -> route -> probe on the owner -> route back -> reduce with the W-rank exchange emulated in
one process: W partition stores on one GPU, the same routing helpers the torch.distributed path uses (as
tests/test_gpu_partitioned.py does it).  A helper module of the suite, not a test file."""
import numpy as np
import torch

import genestrip_amd as ga
from genestrip_amd import distributed as gd


def run(stores, k, seq, off, device_routing):
    """seq / off: a host batch (uint8, uint64[n + 1]); stores: the W partition stores, rank order.
    Returns dict(parts = per rank dict(table, dtable, class_vi, flags) in read order,
                 keys = per rank the int64 keys gs_match_encode wrote (one per k-mer position of the rank's read shard),
                 bounds = per rank (first read, end read),
                 probed = per owner (keys it received int64, nodes gs_match_probe_keys answered int32))"""
    world = len(stores)
    n = len(off) - 1
    dev = torch.device("cuda")
    ms = [ga.FastqKMerMatcher(s) for s in stores]
    bounds = [gd.shard_bounds(n, r, world) for r in range(world)]
    shard = []
    for lo, hi in bounds:
        dseq = torch.from_numpy(seq[int(off[lo]):int(off[hi])].copy()).to(dev) if off[hi] > off[lo] else torch.zeros(1, dtype=torch.uint8, device=dev)
        doff = torch.from_numpy((off[lo:hi + 1] - off[lo]).astype(np.int64)).to(dev)
        shard.append((dseq, doff, hi - lo, lo))
    plans = []
    for r, (dseq, doff, nr, lo) in enumerate(shard):
        pos_off = gd.position_offsets(doff, k)
        nk = int(pos_off[-1].item())
        keys = torch.empty(max(nk, 1), dtype=torch.int64, device=dev)
        ms[r].encode(dseq, doff, pos_off, keys, nr)
        ms[r].sync()
        early = None
        if device_routing:  # gs_route_keys: counting sort on the device
            send = torch.empty(max(nk, 1), dtype=torch.int64, device=dev)
            idx = torch.empty(max(nk, 1), dtype=torch.int32, device=dev)
            early = torch.full((max(nk, 1),), -9, dtype=torch.int32, device=dev) if r % 2 == 0 else None
            counts = np.array(ms[r].route_keys(keys, nk, world, send, idx, early), dtype=np.int64)
            send = send[:int(counts.sum())]
        else:               # the same step with torch ops
            idx, send, counts = gd.plan_routing(keys[:nk], world)
            counts = counts.cpu().numpy()
        plans.append((pos_off, nk, idx, send, counts, keys, early))
    starts = [np.concatenate([[0], np.cumsum(p[4])]) for p in plans]
    node_back = [[None] * world for _ in range(world)]
    probed = []
    for j in range(world):  # all-to-all #1: keys to their owners
        recv = torch.cat([plans[i][3][starts[i][j]:starts[i][j + 1]] for i in range(world)])
        nodes = torch.empty(max(recv.numel(), 1), dtype=torch.int32, device=dev)
        ms[j].probe_keys(recv, nodes, recv.numel())
        ms[j].sync()
        probed.append((recv.cpu().numpy(), nodes[:recv.numel()].cpu().numpy()))
        o = 0
        for i in range(world):  # all-to-all #2: nodes back to the home ranks
            c = int(plans[i][4][j])
            node_back[i][j] = nodes[o:o + c]
            o += c
    parts = []
    for r, (dseq, doff, nr, lo) in enumerate(shard):
        pos_off, nk, idx, _, _, keys, early = plans[r]
        back = torch.cat(node_back[r])
        if device_routing:
            # both ways of filling in the unrouted positions: by gs_route_keys already, or by gs_unroute_nodes
            nodes = early if early is not None else torch.empty(max(nk, 1), dtype=torch.int32, device=dev)
            ms[r].unroute_nodes(None if early is not None else keys, idx, back, back.numel(), nodes, nk)
        else:
            nodes = gd.scatter_nodes(back, idx, max(nk, 1), keys)
        cv = torch.full((max(nr, 1),), -1, dtype=torch.int32, device=dev)
        fl = torch.zeros(max(nr, 1), dtype=torch.uint8, device=dev)
        ms[r].reduce(dseq, doff, pos_off, nodes, nr, first_read_no=lo, class_vi=cv, flags=fl)
        t, d = ms[r].finish()
        parts.append(dict(table=t, dtable=d, class_vi=cv[:nr].cpu().numpy(), flags=fl[:nr].cpu().numpy()))
    for m in ms:
        m.close()
    return dict(parts=parts, keys=[p[5][:p[1]].cpu().numpy() for p in plans], bounds=bounds, probed=probed)
