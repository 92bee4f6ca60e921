"""Times of the store read back (gs_db_value_counts, gs_dbexport_*, gs_host_db2fastq) at three store sizes (developer tool):

    python tools/db_export_rate.py [--genera 0,25,250] [--out DIR]

genera 0 = bench.py's store (SynthDB defaults), 25 -> ~47 M k-mers, 250 -> ~473 M k-mers (BASELINE.json configs[4]); every store is
built on the device from its synthetic genomes (gs_dbbuild + gs_dbbuild_to_db).  Per size: value counts (one decode pass), export
(two decode passes + the radix sort of the pairs), fetch to host memory, and db2fastq to a plain and a .gz file -- of the whole
store up to 50 M k-mers, above that of the largest genus subtree (the whole 473 M-k-mer store is ~47 GB of FASTQ text).  Every call
is synchronous, so a host clock around it is its time; each is run once untimed first.  One JSON line per size.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host, synth  # noqa: E402


def _timed(fn, reps=3):
    fn()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, r


def _store(genera):
    import torch
    db = synth.SynthDB(k=31, genera=genera, species_per_genus=20, build=False) if genera else synth.SynthDB(k=31, build=False)
    g = torch.from_numpy(db.genomes).cuda()
    off = torch.arange(db.genomes.shape[0] + 1, dtype=torch.int64, device="cuda") * db.genomes.shape[1]
    b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
    b.add(g.reshape(-1), off, db.species_vi, update=False)
    b.add(g.reshape(-1), off, db.species_vi, update=True)
    store = b.to_store()
    b.close()
    del g, off
    torch.cuda.empty_cache()
    return db, store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genera", default="0,25,250")
    ap.add_argument("--out", default=None, help="directory for the FASTQ files (deleted after timing); default: a temporary one")
    args = ap.parse_args()
    out_dir = args.out or tempfile.mkdtemp(prefix="gs_db2fastq_")
    for genera in [int(x) for x in args.genera.split(",")]:
        db, store = _store(genera)
        info = store.info
        res = {"genera": genera, "n_stored": int(info.n_stored), "n_in_records": int(info.n_in_records),
               "store_bytes": int(info.rec_bytes + info.table_bytes + info.gate_bytes + info.mgate_bytes)}
        t, counts = _timed(store.value_counts)
        res["value_counts_s"] = t
        res["decode_bytes_per_s"] = (info.rec_bytes + info.table_bytes) / t

        def create():
            x = ga.binding.C.c_void_p()
            n = ga.binding.C.c_int64(0)
            ga.binding._check(ga.lib().gs_dbexport_create(ga.binding.C.byref(x), store.h, -1, 1, ga.binding.C.byref(n)))
            return x, n.value
        t, (x, n) = _timed(lambda: _destroying(create))
        res["export_create_s"] = t  # two decode passes + sort (+ allocation)
        x, n = create()
        kmers = np.empty(n, dtype=np.int64)
        vals = np.empty(n, dtype=np.int32)
        t0 = time.perf_counter()
        ga.binding._check(ga.lib().gs_dbexport_fetch(x, kmers.ctypes.data_as(ga.binding.C.c_void_p), vals.ctypes.data_as(ga.binding.C.c_void_p), ga.MEM_HOST))
        res["fetch_host_s"] = time.perf_counter() - t0
        res["fetch_bytes"] = 12 * n
        ga.lib().gs_dbexport_destroy(x)
        assert n == info.n_stored and np.all(np.diff(kmers) > 0) and np.array_equal(np.bincount(vals, minlength=len(counts)), counts)
        del kmers, vals
        if info.n_stored <= 50_000_000:
            sel, desc, scope = None, True, "total"
        else:
            genus = np.flatnonzero(db.parent_vi == 0)
            sub = np.array([counts[(db.parent_vi == g_) | (np.arange(db.n_values) == g_)].sum() for g_ in genus])
            sel, desc, scope = int(genus[np.argmax(sub)]), True, "largest genus subtree"
        res["db2fastq_scope"] = scope
        for suffix in ("fastq", "fastq.gz"):
            path = os.path.join(out_dir, "db2fastq_%d.%s" % (genera, suffix))
            t, nw = _timed(lambda: host.db2fastq(store, db.taxids, "rate", path, select=sel, with_desc=desc), reps=1)
            size = os.path.getsize(path)
            res["db2fastq_" + suffix.replace(".", "_")] = {"records": nw, "file_bytes": size, "s": t}
            os.unlink(path)
        store.close()
        print(json.dumps(res), flush=True)
    if not args.out:
        os.rmdir(out_dir)


def _destroying(create):
    x, n = create()
    ga.lib().gs_dbexport_destroy(x)
    return x, n


if __name__ == "__main__":
    main()
