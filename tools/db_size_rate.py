"""Sizing rate (developer tool): the counting pass of gs_dbsize (one byte read per base, nothing written per k-mer) and its
distinct pass (keys only, radix sort, heads of runs) over synthetic genomes, alternating in one process with gs_dbbuild on the
same regions; the counting kernel alone (device events) beside the builder's k-mer kernel on the same bytes (the builder's add
call of a device batch is that kernel plus one counter read).  Medians and spreads over the repeats after a warm-up round.
    python tools/db_size_rate.py [--repeats N] [genera ...]      (20 species per genus, 100 kbp each: 25 -> ~47 M, 250 -> ~473 M k-mers)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import synth  # noqa: E402

args = sys.argv[1:]
repeats = 5
if args and args[0] == "--repeats":
    repeats = int(args[1])
    args = args[2:]


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


for genera in [int(x) for x in args] or [25, 250]:
    db = synth.SynthDB(genera=genera, species_per_genus=20, build=False)
    g = db.genomes
    bases = int(g.size)
    dseq = torch.from_numpy(np.ascontiguousarray(g).reshape(-1)).cuda()
    doff = torch.arange(g.shape[0] + 1, dtype=torch.int64, device="cuda") * g.shape[1]
    torch.cuda.synchronize()
    count_s, kernel_ms, keep_s, keep_kernel_ms, sort_ms, heads_ms, build_add_s, build_finish_s = [], [], [], [], [], [], [], []
    result = {}
    for rep in range(repeats + 1):  # (round 0 pays allocations and kernel loading and is dropped)
        t0 = time.time()
        s = ga.DeviceDbSizer(31, db.n_values, hist_bits=12)
        s.add(dseq, doff, db.species_vi)
        t, per_value, hist = s.counts()
        dt = time.time() - t0
        st = s.stats()
        s.close()
        t0 = time.time()
        d = ga.DeviceDbSizer(31, db.n_values, hist_bits=12, radix_bits=20, keep_keys=True)
        d.add(dseq, doff, db.species_vi)
        t1 = time.time()
        n_distinct, buckets = d.distinct()
        t2 = time.time()
        sd = d.stats()
        d.close()
        t3 = time.time()
        b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
        b.add(dseq, doff, db.species_vi, update=False)
        t4 = time.time()
        n_kmers = b.finish_count()
        t5 = time.time()
        b.close()
        ga.lib().gs_device_cache_trim()
        assert n_kmers == n_distinct == int(buckets.sum()) and t.included == int(hist.sum()) == int(per_value.sum())
        if rep == 0:
            continue
        count_s.append(dt)
        kernel_ms.append(st.ms_count)
        keep_s.append(t1 - t0)
        keep_kernel_ms.append(sd.ms_count)
        sort_ms.append(sd.ms_sort)
        heads_ms.append(sd.ms_heads)
        build_add_s.append(t4 - t3)
        build_finish_s.append(t5 - t4)
        result = {"included": t.included, "dust": t.dust, "distinct": n_distinct, "bytes_peak": sd.bytes_peak,
                  "bytes_peak_per_key": round(sd.bytes_peak / max(sd.n_keys, 1), 2), "plan_ranges_at_1GiB_of_pairs": len(
                      ga.plan_ranges(hist, 12, 31, (1 << 30) // 40))}
    print(json.dumps({
        "genera": genera, "bases": bases, **result,
        "count_pass_s": spread(count_s), "count_pass_Mbases_s": spread([bases / x / 1e6 for x in count_s]),
        "count_kernel_ms": spread(kernel_ms), "count_kernel_GB_s": spread([bases / x / 1e6 for x in kernel_ms]),
        "keep_add_s": spread(keep_s), "keep_kernel_ms": spread(keep_kernel_ms), "distinct_sort_ms": spread(sort_ms),
        "distinct_heads_ms": spread(heads_ms),
        "build_add_s (k-mer kernel + counter read)": spread(build_add_s), "build_finish_s": spread(build_finish_s)}))
    del dseq, doff
