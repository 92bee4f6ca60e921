"""Store quality rate (developer tool): the dbquality pass (gs_dbquality: k-mer pairs, two radix sorts, store decode, merge join +
counts) over the genomes a store was built from, beside gs_dbbuild on the same genomes in the same session and, on a sample, the
CPU reference of tests/qualitycheck.py.
    python tools/db_quality_rate.py [--ranges N] [genera ...]      (0 = the bench store; else 20 species per genus, 100 kbp each)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import genestrip_amd as ga  # noqa: E402
import qualitycheck as qc  # noqa: E402
from genestrip_amd import synth  # noqa: E402
from genestrip_amd.binding import kmer_ranges  # noqa: E402

args = sys.argv[1:]
n_ranges = 1
if args and args[0] == "--ranges":
    n_ranges = int(args[1])
    args = args[2:]

for genera in [int(x) for x in args] or [0, 25, 250]:
    db = synth.SynthDB(genera=genera, species_per_genus=20, build=False) if genera else synth.SynthDB(build=False)
    g = db.genomes
    bases = int(g.size)
    dseq = torch.from_numpy(np.ascontiguousarray(g).reshape(-1)).cuda()
    doff = torch.arange(g.shape[0] + 1, dtype=torch.int64, device="cuda") * g.shape[1]
    torch.cuda.synchronize()
    build, quality = [], []
    store = None
    for rep in range(2):  # (the first round pays allocations and kernel loading)
        t0 = time.time()
        b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
        b.add(dseq, doff, db.species_vi, update=False)
        b.add(dseq, doff, db.species_vi, update=True)
        t1 = time.time()
        n_kmers = b.finish_count()
        t2 = time.time()
        if store is None:
            store = b.to_store()
        b.close()
        build.append({"add_s": round(t1 - t0, 4), "finish_s": round(t2 - t1, 4), "total_s": round(t2 - t0, 4)})
    for rep in range(2):
        t0 = time.time()
        q = ga.DeviceDbQuality(store)
        counts = np.zeros((db.n_values, 3), np.int64)
        phases = {"pairs_ms": 0.0, "sort_ms": 0.0, "store_decode_ms": 0.0, "join_count_ms": 0.0}
        pairs = distinct = 0
        for i, (lo, hi) in enumerate(kmer_ranges(31, n_ranges)):
            if n_ranges > 1:
                q.set_range(lo, hi)
            q.add(dseq, doff, db.species_vi)
            c, p = q.finish()
            st = q.stats()
            counts[:, [0, 2]] += c[:, [0, 2]]
            counts[p > 0, 1] = c[p > 0, 1]
            phases["pairs_ms"] += st.ms_pairs
            phases["sort_ms"] += st.ms_sort
            phases["join_count_ms"] += st.ms_join
            if i == 0:
                phases["store_decode_ms"] = st.ms_decode
            pairs += st.n_pairs
            distinct += st.n_distinct
        q.close()
        dt = time.time() - t0
        quality.append({"total_s": round(dt, 4), **{k: round(v, 2) for k, v in phases.items()}})
    sp = counts[db.species_vi]
    # a store against its own sources: every genome k-mer is stored on its leaf's path
    ok = bool((sp[:, 0] == sp[:, 2]).all() and (sp[:, 0] > 0).all() and (sp[:, 1] >= sp[:, 0]).all() and distinct == sp[:, 2].sum())
    # CPU reference on the first 40 genomes (single thread), against the store's own arrays
    ns = min(40, g.shape[0])
    cpu = None
    if n_kmers <= 60_000_000:
        sk, sv = store.export()
        regions = [(g[i].tobytes(), int(db.species_vi[i])) for i in range(ns)]
        t0 = time.time()
        ref = qc.reference_counts(31, sk, sv, db.parent_vi, regions)
        cpu = round(ns * g.shape[1] / (time.time() - t0) / 1e6, 2)
        ok = ok and bool(np.array_equal(ref["counts"][db.species_vi[:ns]][:, [0, 2]], sp[:ns][:, [0, 2]]))
    print(json.dumps({"genomes": int(g.shape[0]), "bases": bases, "store_kmers": int(n_kmers), "pairs": int(pairs), "distinct_pairs": int(distinct),
                      "ranges": n_ranges, "consistent": ok, "gs_dbbuild": build, "gs_dbquality": quality,
                      "quality_mbases_per_s": round(bases / quality[-1]["total_s"] / 1e6, 1),
                      "build_mbases_per_s": round(bases / build[-1]["total_s"] / 1e6, 1),
                      "quality_over_build": round(quality[-1]["total_s"] / build[-1]["total_s"], 2),
                      "cpu_reference_mbases_per_s_1_thread": cpu}), flush=True)
    store.close()
    del dseq, doff
