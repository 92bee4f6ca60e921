"""Store quality end to end on the GPU: a store and the genomes it was built from -> per-taxon true positives, precision and recall,
the CSV of the reference's dbquality goal.

    python examples/db_quality.py --store my.gsstore --tree nodes.tsv --map files.tsv --out quality.csv genomes/*.fasta

nodes.tsv: one line per tax node IN THE ORDER OF THE STORE'S VALUE INDICES (as given to examples/build_db.py),
`taxid <tab> parent taxid [<tab> rank [<tab> name]]`; files.tsv: `file name <tab> taxid`, the leaf node of every record of that
FASTA file (without --map: the taxid in the first header field `>taxid|...`).  Without arguments a synthetic collection is built
into a store first, so the script runs as is:

    python examples/db_quality.py --demo

(Which node is a file's leaf in the reference -- id nodes, file nodes, data children -- is host logic and not part of this example.)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host, synth  # noqa: E402
from build_db import read_fasta  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fasta", nargs="*")
    ap.add_argument("--store")
    ap.add_argument("--tree")
    ap.add_argument("--map")
    ap.add_argument("--out", default="quality.csv")
    ap.add_argument("--max-dust", type=int, default=-1)
    ap.add_argument("--step", type=int, default=1)
    ap.add_argument("--demo", action="store_true")
    args = ap.parse_args()
    if not args.demo and not (args.store and args.tree and args.fasta):
        ap.error("give --demo, or --store, --tree and FASTA files")

    if args.demo:
        db = synth.SynthDB(genera=5, species_per_genus=8, genome_len=200_000, build=False)
        parent_vi, taxids = db.parent_vi, db.taxids
        depth = [0 if p < 0 else 1 if parent_vi[p] < 0 else 2 for p in parent_vi]
        ranks = [("no rank", "genus", "species")[d] for d in depth]
        names = ["%s %s" % (r, t) for r, t in zip(ranks, taxids)]
        regions = [(db.genomes[i].tobytes(), int(db.species_vi[i])) for i in range(db.genomes.shape[0])]
        seq, off, nodes = _pack(regions)
        b = ga.DeviceDbBuilder(31, db.n_values, parent_vi, max_dust=args.max_dust, step_size=args.step)
        b.add(seq, off, nodes, update=False)
        b.add(seq, off, nodes, update=True)
        store = b.to_store()
        b.close()
    else:
        rows = [line.rstrip("\n").split("\t") for line in open(args.tree) if line.strip()]
        taxids = [f[0] for f in rows]
        vi = {t: i for i, t in enumerate(taxids)}
        parent_vi = np.array([vi[f[1]] if len(f) > 1 and f[1] and f[1] != f[0] else -1 for f in rows], dtype=np.int32)
        ranks = [f[2] if len(f) > 2 else "no rank" for f in rows]
        names = [f[3] if len(f) > 3 else f[0] for f in rows]
        of_file = {}
        if args.map:
            of_file = dict(line.rstrip("\n").split("\t")[:2] for line in open(args.map) if line.strip())
        regions = []
        for path in args.fasta:
            for name, s in read_fasta(path):
                tax = of_file.get(os.path.basename(path)) if args.map else name.split("|")[0].split()[0]
                regions.append((s, vi.get(tax, -1)))  # (-1: no leaf node in the store's tree, the region counts nothing)
        seq, off, nodes = _pack(regions)
        store = ga.DeviceKMerStore.load(args.store)
        if store.n_values != len(taxids):
            sys.exit("the tree has %d nodes, the store %d values" % (len(taxids), store.n_values))

    t0 = time.time()
    q = ga.DeviceDbQuality(store, max_dust=args.max_dust, step_size=args.step)
    q.add(seq, off, nodes)
    counts, present = q.finish()
    st = q.stats()
    q.close()
    dt = time.time() - t0
    host.write_quality_csv(args.out, parent_vi, taxids, counts, present, names=names, ranks=ranks)
    tp, tp_fp, tp_fn = (int(x) for x in counts[present > 0].sum(axis=0))
    print("%d regions, %.1f Mbases against %d stored k-mers in %.2f s (%.0f Mbases/s): %d distinct (k-mer, leaf) pairs, %d stored; "
          "%d taxa, precision %.4f, recall %.4f over all of them; %s written" %
          (len(regions), len(seq) / 1e6, st.n_store, dt, len(seq) / dt / 1e6, st.n_distinct, st.n_found, int(present.sum()),
           tp / max(tp_fp, 1), tp / max(tp_fn, 1), args.out))
    store.close()


def _pack(regions):
    seq = np.frombuffer(b"".join(s for s, _ in regions), dtype=np.uint8)
    if len(seq) == 0:
        seq = np.zeros(1, dtype=np.uint8)
    off = np.cumsum([0] + [len(s) for s, _ in regions]).astype(np.uint64)
    return seq, off, np.array([n for _, n in regions], dtype=np.int32)


if __name__ == "__main__":
    main()
