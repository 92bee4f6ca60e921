"""The index goal from a device store (gs_bloom_build_db) against the path a caller had to compose before it (developer tool):

    python tools/index_build_rate.py [--genera 0,25,250] [--repeats N]

genera as in tools/db_export_rate.py: 0 = bench.py's store, 25 -> ~47 M k-mers, 250 -> ~473 M k-mers; every store is built on the
device from its synthetic genomes.  Requested set: all species.  Per store and kind (XOR at 1e-8, blocked) the two paths run by
turns on the same store in one process, `--repeats` times each after one untimed turn (at least five); every call is synchronous,
so a host clock around a path is its time.  Reported: the fastest run and the spread (slowest - fastest) of each path.

  composed   gs_dbexport_create(-1) [two decode passes + the radix sort of all pairs] -> gs_dbexport_fetch into device arrays ->
             mask by value on the device -> gs_bloom_build from device memory.  For a blocked filter the composed path is the export
             alone: gs_bloom_build makes no blocked filter, so the figure is a lower bound of what a caller would have paid.
  from store gs_bloom_build_db.

GS_INDEX_TRACE=1 is set for one more build per kind: the library then prints its count pass and put pass between events (stderr).
`existing_put_call_s` is gs_bloom_build alone on the selected keys in device memory (filter allocation, memset and the existing
put kernel).  Memory beyond the store and the filter is computed from what each path allocates: the export holds 12 B per stored
k-mer, twice that while it sorts, the caller's device copy another 12 B and the selected keys 8 B each; the call on the store
holds the requested bitmap and two counters.  One JSON line per store and kind.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd.binding import _check  # noqa: E402
from db_export_rate import _store  # noqa: E402


def _export_to_device(store):
    import torch
    x, n = C.c_void_p(), C.c_int64(0)
    _check(ga.lib().gs_dbexport_create(C.byref(x), store.h, -1, 0, C.byref(n)))
    try:
        keys = torch.empty(n.value, dtype=torch.int64, device="cuda")
        vals = torch.empty(n.value, dtype=torch.int32, device="cuda")
        _check(ga.lib().gs_dbexport_fetch(x, C.c_void_p(keys.data_ptr()), C.c_void_p(vals.data_ptr()), ga.MEM_DEVICE))
    finally:
        ga.lib().gs_dbexport_destroy(x)
    return keys, vals


def _composed(store, req_dev, kind, fpp):
    import torch
    keys, vals = _export_to_device(store)
    if kind == ga.BLOOM_BLOCKED:
        torch.cuda.synchronize()
        return None
    sel = keys[req_dev[vals.long()]]
    del keys, vals
    bloom = ga.DeviceBloomFilter.build(sel, fpp=fpp, kind=kind)  # (expected_insertions = the count, as the goal sizes it)
    return bloom


def _clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--genera", default="0,25,250")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    reps = max(args.repeats, 5)
    for genera in [int(x) for x in args.genera.split(",")]:
        db, store = _store(genera)
        info = store.info
        requested = np.zeros(db.n_values, dtype=np.uint8)
        requested[db.species_vi] = 1
        req_dev = torch.from_numpy(requested != 0).cuda()
        for name, kind, fpp in (("xor-1e-8", ga.BLOOM_XOR, 1e-8), ("blocked", ga.BLOOM_BLOCKED, 0.01)):
            times = {"composed": [], "from_store": []}
            words = {}
            for turn in range(reps + 1):  # by turns; turn 0 is untimed
                for path in ("composed", "from_store"):
                    if path == "composed":
                        dt, bloom = _clock(lambda: _composed(store, req_dev, kind, fpp))
                    else:
                        dt, bloom = _clock(lambda: ga.DeviceBloomFilter.from_store(store, requested, kind=kind, fpp=fpp))
                    if turn > 0:
                        times[path].append(dt)
                    if bloom is not None:
                        if turn == 0 and info.n_stored <= 60_000_000:
                            words[path] = bloom.get()
                        n_sel = bloom.info().n_inserted
                        bloom.close()
            if len(words) == 2:  # the two paths build the same filter
                assert words["composed"][0] == words["from_store"][0] and np.array_equal(words["composed"][2], words["from_store"][2])
            res = {"genera": genera, "kind": name, "n_stored": int(info.n_stored), "n_selected": int(n_sel), "repeats": reps}
            for path, ts in times.items():
                res[path + "_s"] = {"min": min(ts), "spread": max(ts) - min(ts), "all": [round(t, 5) for t in ts]}
            res["from_store_over_composed"] = res["from_store_s"]["min"] / res["composed_s"]["min"]
            if kind != ga.BLOOM_BLOCKED:
                keys, vals = _export_to_device(store)
                sel = keys[req_dev[vals.long()]]
                del keys, vals
                ts = []
                for turn in range(reps + 1):
                    dt, bloom = _clock(lambda: ga.DeviceBloomFilter.build(sel, fpp=fpp, kind=kind))
                    bloom.close()
                    if turn > 0:
                        ts.append(dt)
                res["existing_put_call_s"] = {"min": min(ts), "spread": max(ts) - min(ts)}
                del sel
            os.environ["GS_INDEX_TRACE"] = "1"  # the library prints the two passes between events
            ga.DeviceBloomFilter.from_store(store, requested, kind=kind, fpp=fpp).close()
            del os.environ["GS_INDEX_TRACE"]
            n = int(info.n_stored)
            res["extra_device_bytes"] = {"composed_peak": 24 * n + 12 * n + (0 if kind == ga.BLOOM_BLOCKED else 8 * int(n_sel)),
                                         "composed_held": 12 * n + (0 if kind == ga.BLOOM_BLOCKED else 8 * int(n_sel)),
                                         "from_store": 4 * ((db.n_values + 31) // 32) + 16}
            print(json.dumps(res), flush=True)
            torch.cuda.empty_cache()
        store.close()


if __name__ == "__main__":
    main()
