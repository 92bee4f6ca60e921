"""DB construction end to end on the GPU: genome FASTA files -> (k-mer, lowest common ancestor) arrays -> store layout -> native
store file, the way FillDBGoal + DBGoal do it with two walks over the collection on the CPU.

    python examples/build_db.py --out my.gsstore --tree nodes.tsv genomes/*.fasta

nodes.tsv: one line per tax node, `taxid <tab> parent taxid` (the root's parent is itself or empty); every FASTA file is one
genome whose records all belong to the taxid in its first header field `>taxid|...` or, with --by-file, to the taxid that is the
file's basename.  Without arguments a synthetic collection is used (genestrip_amd.synth), so the script runs as is:

    python examples/build_db.py --demo

(What decides which regions count in the reference -- accession maps, RefSeq categories, per-taxid limits -- is host logic and not
part of this example; java/src/.../refseq/GpuStoreFastaReader.java shows the reference-side reader.)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host, synth  # noqa: E402


def header_taxid(header):
    """this example's rule: the first field of `>taxid|...` (a header line as the device hands it out: '>' first, no line end)"""
    name = header[1:].strip().decode("latin1")
    fields = name.split("|")[0].split()
    return fields[0] if fields else ""


def add_files(builder, paths, vi, by_file, update):
    """one walk over the FASTA files (plain, gzip or BGZF): the records are found and their bases gathered on the device
    (host.genome_files), this callback decides from the header lines which of them count and for which node -> GenomeTotals"""
    def resolve(file, _first_record, headers):
        tax_of_file = os.path.splitext(os.path.basename(paths[file]))[0]
        return [vi.get(tax_of_file if by_file else header_taxid(h), -1) for h in headers]

    return host.genome_files(paths, resolve, lambda seq, off, nodes: builder.add(seq, off, nodes, update=update))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("fasta", nargs="*")
    ap.add_argument("--tree")
    ap.add_argument("--by-file", action="store_true")
    ap.add_argument("--out", default="built.gsstore")
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--max-dust", type=int, default=-1)
    ap.add_argument("--demo", action="store_true")
    args = ap.parse_args()
    if not args.demo and not (args.tree and args.fasta):
        ap.error("give --demo, or --tree and FASTA files")

    t0 = time.time()
    if args.demo:
        db = synth.SynthDB(k=args.k, genera=5, species_per_genus=8, genome_len=200_000)
        parent_vi, n_values = db.parent_vi, db.n_values
        regions = [(db.genomes[i].tobytes(), int(db.species_vi[i])) for i in range(db.genomes.shape[0])]
        taxids = db.taxids
    else:
        ids, parents = [], {}
        for line in open(args.tree):
            f = line.rstrip("\n").split("\t")
            if f and f[0]:
                ids.append(f[0])
                parents[f[0]] = f[1] if len(f) > 1 and f[1] and f[1] != f[0] else None
        vi = {t: i for i, t in enumerate(ids)}
        parent_vi = np.array([vi[parents[t]] if parents[t] is not None else -1 for t in ids], dtype=np.int32)
        n_values, taxids = len(ids), ids
    t_read = time.time() - t0

    t0 = time.time()
    b = ga.DeviceDbBuilder(args.k, n_values, parent_vi, max_dust=args.max_dust)
    if args.demo:
        seq = np.frombuffer(b"".join(s for s, _ in regions), dtype=np.uint8)
        off = np.cumsum([0] + [len(s) for s, _ in regions]).astype(np.uint64)
        nodes = np.array([n for _, n in regions], dtype=np.int32)
        n_regions, n_bases = len(regions), len(seq)
        b.add(seq, off, nodes, update=False)  # FillDBGoal: the k-mers of these regions are stored ...
        b.add(seq, off, nodes, update=True)   # ... DBGoal: and every region moves the k-mers it shares towards the common ancestor
    else:  # the same two walks over the files, as the reference makes them; the text never becomes Python objects
        t = add_files(b, args.fasta, vi, args.by_file, update=False)
        add_files(b, args.fasta, vi, args.by_file, update=True)
        n_regions, n_bases = t.kept_records, t.kept_bases
        t_walks = time.time() - t0
    n_kmers = b.finish_count()
    store = b.to_store()                  # the layout (records, overflow table, gate) without leaving the GPU
    b.close()
    t_build = time.time() - t0
    info = store.info
    store.save(args.out)
    if args.demo:
        head = "%d regions, %.1f Mbases read in %.2f s; %d distinct k-mers with LCA values + store layout in %.2f s " % (
            n_regions, n_bases / 1e6, t_read, n_kmers, t_build)
    else:  # (the files are read inside the two walks: their time is part of the build's)
        head = "%d regions, %.1f Mbases; two walks over the files, %d distinct k-mers with LCA values and store layout in %.2f s, %.2f s of it the walks " % (
            n_regions, n_bases / 1e6, n_kmers, t_build, t_walks)
    print(head + "(%.0f Mbases/s); %d k-mers in records, %d in the overflow table; %s written (%.1f MB)" %
          (n_bases / t_build / 1e6, info.n_in_records, info.n_stored - info.n_in_records, args.out, os.path.getsize(args.out) / 1e6))
    if args.demo:  # the store answers reads drawn from its genomes
        rs, ro = synth.reads_host(db.genomes, 20000, read_len=150, seed=1)
        m = ga.FastqKMerMatcher(store)
        m.submit(rs, ro.astype(np.uint64), 0)
        table, _ = m.finish()
        m.close()
        top = np.argsort(-table[:, 0])[:3]
        print("20000 reads from the genomes: %d classified; most reads: %s" %
              (int(table[:, 0].sum()), ", ".join("taxid %s: %d" % (taxids[i], table[i, 0]) for i in top)))
    store.close()


if __name__ == "__main__":
    main()
