"""Streaming update rate (developer tool): a store built from the fill regions of synthetic genomes, then the whole collection
streamed past it in batches (gs_dbupdate), beside the one-shot gs_dbbuild of the same fill + update regions in the same process,
alternating, and the CPU restatement's update on a sample.   python tools/db_update_rate.py [--repeats N] [--batch GENOMES] [genera ...]
(20 species per genus, 100 kbp each: 25 genera = about 47 M k-mers, 250 = about 473 M).  One JSON line per size.  Host clock
around synchronous calls; the phase times are gs_dbupdate_stats (device events around the kernels of every slice)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import synth  # noqa: E402
from oracle import gs_oracle as orc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("genera", nargs="*", type=int)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--batch", type=int, default=50, help="genomes per gs_dbupdate_add")
ap.add_argument("--slice", type=int, default=0, help="gs_dbupdate_set_slice (0: the default)")
args = ap.parse_args()


def spread(xs):
    return {"min": round(min(xs), 4), "median": round(float(np.median(xs)), 4), "max": round(max(xs), 4)}


for genera in args.genera or [25, 250]:
    db = synth.SynthDB(genera=genera, species_per_genus=20)
    g = db.genomes
    n_genomes, glen = g.shape
    bases = int(g.size)
    dseq = torch.from_numpy(np.ascontiguousarray(g).reshape(-1)).cuda()
    doff = torch.arange(n_genomes + 1, dtype=torch.int64, device="cuda") * glen
    torch.cuda.synchronize()

    def one_shot():
        t0 = time.time()
        b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
        b.add(dseq, doff, db.species_vi, update=False)
        b.add(dseq, doff, db.species_vi, update=True)
        n = b.finish_count()
        dt = time.time() - t0
        b.close()
        return dt, n

    def fill_store():
        b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
        b.add(dseq, doff, db.species_vi, update=False)
        u = ga.DeviceDbUpdater.from_builder(b)
        b.close()
        return u

    def stream(check=False):
        u = fill_store()
        if args.slice:
            u.set_slice(args.slice)
        t0 = time.time()
        for a in range(0, n_genomes, args.batch):
            e = min(a + args.batch, n_genomes)
            u.add(dseq[a * glen:e * glen], doff[:e - a + 1], db.species_vi[a:e])
        moved = u.finish()
        dt = time.time() - t0
        st = u.stats()
        ok = None
        if check:
            k, v = u.fetch()
            ok = bool(np.array_equal(k, db.kmers) and np.array_equal(v, db.value_idx))
        u.close()
        return dt, moved, st, ok

    one_shot()  # warm-up of both paths: code objects, rocPRIM, the allocator's blocks
    _, _, _, ok = stream(check=True)
    shot, strm, kmers_ms, lookup_ms, begin_ms = [], [], [], [], []
    for _ in range(args.repeats):  # alternating
        shot.append(one_shot()[0])
        dt, moved, st, _ = stream()
        strm.append(dt)
        kmers_ms.append(st.ms_kmers)
        lookup_ms.append(st.ms_lookup)
        begin_ms.append(st.ms_begin)
    # CPU restatement's update on the first 40 genomes against the store of those genomes (single thread)
    ns = min(40, n_genomes)
    sseq = np.ascontiguousarray(g[:ns]).reshape(-1)
    soff = (np.arange(ns + 1) * glen).astype(np.uint64)
    ob = orc.DbBuild(31, db.n_values, db.parent_vi)
    ob.fill(sseq, soff, db.species_vi[:ns])
    ob.optimize()
    t0 = time.time()
    ob.update(sseq, soff, db.species_vi[:ns])
    cpu_dt = time.time() - t0
    ob.close()
    print(json.dumps({
        "genomes": n_genomes, "bases": bases, "store_kmers": int(st.n_store), "batch_genomes": args.batch, "repeats": args.repeats,
        "equals_synth_store": ok, "n_pairs": int(st.n_pairs), "n_found": int(st.n_found), "n_moved": int(moved),
        "store_bytes": int(st.store_bytes), "batch_bytes_peak": int(st.batch_bytes_peak),
        "stream_update_s": spread(strm), "stream_mbases_per_s": round(bases / float(np.median(strm)) / 1e6, 1),
        "ms_begin": spread(begin_ms), "ms_kmers": spread(kmers_ms), "ms_lookup": spread(lookup_ms), "ms_finish": round(st.ms_finish, 3),
        "one_shot_fill_plus_update_s": spread(shot), "one_shot_mbases_per_s": round(bases / float(np.median(shot)) / 1e6, 1),
        "cpu_update_mbases_per_s_1_thread": round(ns * glen / cpu_dt / 1e6, 2)}), flush=True)
    del dseq, doff
