"""The updatedb stage as a stream: a finished store is loaded from its file, the regions of a whole genome collection go past it
in batches, and every stored k-mer a region holds moves to the lowest common ancestor of its value and the region's node
(DBGoal on the CPU).  The store stays on the GPU; memory does not grow with the collection.

    python examples/update_db.py --store in.gsstore --tree nodes.tsv genomes/*.fasta --out out.gsstore

nodes.tsv and the FASTA conventions are those of examples/build_db.py (the value indices of the store are the line numbers of
nodes.tsv, as build_db.py assigns them).  Without files a synthetic collection is used, so the script runs as is:

    python examples/update_db.py --demo

The demo builds a store from FILL regions only (every k-mer sits under the first species that holds it), saves it, loads it and
streams the whole collection past it; reads from the core two species of a genus share are classified at a species before and
at the genus afterwards.
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
from build_db import read_fasta  # noqa: E402


def batches(regions, max_bases):
    part, size = [], 0
    for r in regions:
        if part and size + len(r[0]) > max_bases:
            yield part
            part, size = [], 0
        part.append(r)
        size += len(r[0])
    if part:
        yield part


def update(store, regions, batch_bases, max_dust=-1):
    """-> (updated store, stats, seconds)"""
    t0 = time.time()
    u = ga.DeviceDbUpdater.from_store(store, max_dust=max_dust)
    n = 0
    for part in batches(regions, batch_bases):
        seq = np.frombuffer(b"".join(s for s, _ in part), dtype=np.uint8)
        off = np.cumsum([0] + [len(s) for s, _ in part]).astype(np.uint64)
        u.add(seq, off, np.array([v for _, v in part], dtype=np.int32))
        n += 1
    u.finish()
    st = u.stats()
    out = u.to_store()
    u.close()
    return out, st, n, time.time() - t0


def classes(store, seq, off):
    m = ga.FastqKMerMatcher(store)
    cv, _ = m.match_reads(seq, off)
    m.finish()
    m.close()
    return cv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fasta", nargs="*")
    ap.add_argument("--store")
    ap.add_argument("--tree")
    ap.add_argument("--by-file", action="store_true")
    ap.add_argument("--out", default="updated.gsstore")
    ap.add_argument("--max-dust", type=int, default=-1)
    ap.add_argument("--batch-mbases", type=float, default=16.0)
    ap.add_argument("--demo", action="store_true")
    args = ap.parse_args()
    if not args.demo and not (args.store and args.tree and args.fasta):
        ap.error("give --demo, or --store, --tree and FASTA files")
    batch_bases = int(args.batch_mbases * 1e6)

    if args.demo:
        db = synth.SynthDB(k=31, genera=5, species_per_genus=8, genome_len=200_000)
        regions = [(db.genomes[i].tobytes(), int(db.species_vi[i])) for i in range(db.genomes.shape[0])]
        seq = np.frombuffer(b"".join(s for s, _ in regions), dtype=np.uint8)
        off = np.cumsum([0] + [len(s) for s, _ in regions]).astype(np.uint64)
        b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
        b.add(seq, off, db.species_vi, update=False)  # filldb only
        filled = b.to_store()
        b.close()
        path = os.path.join(tempfile.mkdtemp(), "filled.gsstore")
        filled.save(path)
        filled.close()
        args.store = path
    else:
        ids = [line.split("\t")[0] for line in open(args.tree) if line.strip()]
        vi = {t: i for i, t in enumerate(ids)}
        regions = []
        for p in args.fasta:
            for name, s in read_fasta(p):
                tax = os.path.splitext(os.path.basename(p))[0] if args.by_file else name.split("|")[0].split()[0]
                if tax in vi:
                    regions.append((s, vi[tax]))

    store = ga.DeviceKMerStore.load(args.store)
    updated, st, n, dt = update(store, regions, batch_bases, args.max_dust)
    updated.save(args.out)
    bases = sum(len(s) for s, _ in regions)
    print("%d regions, %.1f Mbases in %d batches past a store of %d k-mers in %.2f s (%.0f Mbases/s): %d k-mers found, %d values moved; "
          "device memory: store %.1f MB + %.1f MB per slice; %s written" %
          (len(regions), bases / 1e6, n, st.n_store, dt, bases / dt / 1e6, st.n_found, st.n_moved, st.store_bytes / 1e6,
           st.batch_bytes_peak / 1e6, args.out))
    if args.demo:
        # reads that lie in k-mers the species of a genus share: the values of those k-mers are genus nodes after the update
        shared = np.flatnonzero(np.isin(db.value_idx, db.species_vi, invert=True))
        rs, ro = synth.reads_host(db.genomes, 20000, read_len=150, seed=1)
        before, after = classes(store, rs, ro.astype(np.uint64)), classes(updated, rs, ro.astype(np.uint64))
        is_species = np.isin(before, db.species_vi)
        lifted = is_species & (after >= 0) & ~np.isin(after, db.species_vi)
        print("20000 reads from the genomes (%d of the %d k-mers are shared between genomes): %d classified at a species by the filled "
              "store, of which %d at a genus or above by the updated store" % (len(shared), len(db.kmers), int(is_species.sum()), int(lifted.sum())))
    store.close()
    updated.close()


if __name__ == "__main__":
    main()
