"""The index goal: the Bloom filter of the k-mers a finished store holds for the requested tax ids, built on the GPU from the store
itself (BloomIndexGoal on the CPU) and kept in a native index file for the filter goal.

    python examples/build_index.py --store my.gsstore --taxids-file nodes.tsv --requested 562,1280 --out my.gsindex
                                   [--fpp 1e-8] [--kind xor|murmur|blocked]

--taxids-file: one line per value index of the store, the tax id first (the nodes.tsv of examples/build_db.py will do).  A node is
requested by its own tax id; its descendants are not implied, as in the reference (name them too).  Then, in any later process:

    bloom = genestrip_amd.DeviceBloomFilter.load("my.gsindex")
    genestrip_amd.host.filter_files(bloom, k, ["sample.fastq.gz"], filtered_path="kept.fastq.gz")

Without files a synthetic collection is used, so the script runs as is:

    python examples/build_index.py --demo

The demo builds a store, indexes its species, saves the index, loads it into a fresh handle and filters synthetic reads (half from
the genomes, half random) with it; it prints the accepted count beside the CPU oracle's for the same filter.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import synth  # noqa: E402

KINDS = {"xor": ga.BLOOM_XOR, "murmur": ga.BLOOM_MURMUR, "blocked": ga.BLOOM_BLOCKED}


def build_index(store, requested, kind, fpp, out):
    t0 = time.time()
    bloom = ga.DeviceBloomFilter.from_store(store, requested, kind=kind, fpp=fpp)
    dt = time.time() - t0
    bloom.save(out)
    i = bloom.info()
    print("%d of the store's %d k-mers are requested; %s filter of %d %s (%.1f MB, %d hash%s) built in %.3f s; %s written (%d bytes)" %
          (i.n_inserted, store.info.n_stored, [n for n, v in KINDS.items() if v == i.kind][0], i.bits,
           "buckets" if i.kind == ga.BLOOM_BLOCKED else "bits", 8 * i.n_words / 1e6, i.n_hashes, "" if i.n_hashes == 1 else "es", dt, out,
           os.path.getsize(out)))
    return bloom


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store")
    ap.add_argument("--taxids-file")
    ap.add_argument("--requested", help="comma-separated tax ids")
    ap.add_argument("--out", default="index.gsindex")
    ap.add_argument("--fpp", type=float, default=1e-8)
    ap.add_argument("--kind", choices=sorted(KINDS), default="xor")
    ap.add_argument("--demo", action="store_true")
    args = ap.parse_args()
    if not args.demo and not (args.store and args.taxids_file and args.requested):
        ap.error("give --demo, or --store, --taxids-file and --requested")
    kind = KINDS[args.kind]

    if not args.demo:
        taxids = [line.split("\t")[0].strip() for line in open(args.taxids_file) if line.strip()]
        store = ga.DeviceKMerStore.load(args.store)
        if len(taxids) != store.info.n_values:
            sys.exit("%s names %d tax ids, the store has %d values" % (args.taxids_file, len(taxids), store.info.n_values))
        requested = ga.requested_mask(taxids, [t for t in args.requested.split(",") if t])
        build_index(store, requested, kind, args.fpp, args.out).close()
        store.close()
        return

    from oracle import gs_oracle as orc  # (the demo's yardstick only; the product path has no use for it)
    k = 31
    db = synth.SynthDB(k=k, genera=4, species_per_genus=5, genome_len=100_000)
    store = ga.DeviceKMerStore(k, db.kmers, db.value_idx, db.n_values, db.parent_vi)
    requested = ga.requested_mask(db.taxids, [db.taxids[v] for v in db.species_vi])
    out = os.path.join(tempfile.mkdtemp(), "species.gsindex")
    build_index(store, requested, kind, args.fpp, out).close()
    store.close()

    bloom = ga.DeviceBloomFilter.load(out)  # what a later process does
    n = 20000
    hit, off = synth.reads_host(db.genomes, n // 2, read_len=150, seed=1)
    rng = np.random.default_rng(2)
    seq = np.concatenate([hit, np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n // 2) * 150)]])
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(150)
    accepted = ga.FastqBloomFilter(k, bloom, min_pos_count=0, positive_ratio=0.2).accept_reads(seq, off)
    i = bloom.info()
    bloom.close()

    keys = db.kmers[requested[db.value_idx] != 0]
    ob = orc.Bloom(kind, max(len(keys), 1), args.fpp)
    ob.put_many(keys)
    want = ob.filter_batch(k, 0, 0.2, seq, off)
    print("%d reads (half from the genomes, half random) through the loaded index: %d accepted on the GPU, %d by the CPU oracle's filter "
          "of the same %d k-mers (%s)" % (n, int(accepted.sum()), int(want.sum()), i.n_inserted,
                                          "equal flags" if np.array_equal(accepted, want) else "FLAGS DIFFER"))
    if not np.array_equal(accepted, want) or len(keys) != i.n_inserted:
        sys.exit(1)


if __name__ == "__main__":
    main()
