"""From NCBI's taxonomy files to a store on the GPU: nodes.dmp / names.dmp -> the tree, taxids.txt -> the taxnodes set, a RefSeq
catalog -> the accession map over the tree's ids, genome FASTA files -> regions under the selected nodes, the tree a database
carries -> a k-mer store -> a match with names and ranks (the taxtree and taxnodes goals in front of the chain).

    python examples/taxonomy.py --demo

writes a small dump, a tax id file, a catalog, two FASTA files and some reads, and walks the whole road.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host  # noqa: E402

# id, parent, rank, name
TAXA = [(1, 1, "no rank", "root"), (2, 1, "superkingdom", "Bacteria"), (1224, 2, "phylum", "Pseudomonadota"), (561, 1224, "genus", "Escherichia"),
        (562, 561, "species", "Escherichia coli"), (83333, 562, "strain", "Escherichia coli K-12"), (564, 561, "species", "Escherichia fergusonii"),
        (1239, 2, "phylum", "Bacillota"), (1279, 1239, "genus", "Staphylococcus"), (1280, 1279, "species", "Staphylococcus aureus"),
        (10239, 1, "superkingdom", "Viruses"), (11053, 10239, "species", "Dengue virus 1")]
GENOMES = [("NC_000913.3", 83333), ("NC_011740.1", 564), ("NC_007795.1", 1280), ("NC_001477.1", 11053)]
CATEGORIES, STATUSES = ["bacteria", "viral"], ["REVIEWED", "VALIDATED"]


def write_demo(tmp):
    rng = np.random.default_rng(9)
    p = lambda name: os.path.join(tmp, name)
    open(p("nodes.dmp"), "w").write("".join(f"{t}\t|\t{par}\t|\t{rank}\t|\t\t|\t0\t|\t1\t|\t11\t|\n" for t, par, rank, _ in TAXA))
    names = []
    for t, _, _, name in TAXA:
        names.append(f"{t}\t|\tan older name of {name}\t|\t\t|\tsynonym\t|\n")
        names.append(f"{t}\t|\t{name}\t|\t\t|\tscientific name\t|\n")
    open(p("names.dmp"), "w").write("".join(names))
    # everything below Bacteria down to species, without the Staphylococci; viruses are not asked for
    open(p("taxids.txt"), "w").write("# the demo's request\nBacteria\t2\n-1279  # no Staphylococci\n999999\n")
    open(p("catalog"), "w").write("".join(f"{t}\tSome name\t{acc}\tcomplete|{'viral' if t == 11053 else 'bacteria'}\tREVIEWED\t5000\n" for acc, t in GENOMES))
    seqs = {acc: "".join(rng.choice(list("ACGT"), 5000)) for acc, _ in GENOMES}
    paths = []
    for f in range(2):
        lines = []
        for acc, _ in GENOMES[f::2]:
            lines.append(f">{acc} Some organism, complete genome\n")
            lines += [seqs[acc][i:i + 70] + "\n" for i in range(0, 5000, 70)]
        paths.append(p(f"genomes{f}.fna"))
        open(paths[-1], "w").write("".join(lines))
    reads = [seqs[acc][i:i + 120] for acc, _ in GENOMES for i in range(0, 4800, 400)]
    return p("nodes.dmp"), p("names.dmp"), p("taxids.txt"), p("catalog"), paths, reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--demo", action="store_true")
    if not ap.parse_args().demo:
        ap.error("give --demo")
    with tempfile.TemporaryDirectory() as tmp:
        nodes_path, names_path, taxids_path, catalog_path, fasta_paths, reads = write_demo(tmp)
        # 1. the taxtree goal: chunks of nodes lines are scanned on the device, the tree is made there
        tree, rep = host.taxtree_files(nodes_path, names_path)
        a, names = tree.arrays(), tree.names()
        print("tree: %d nodes, %d reached from the root, deepest at %d; %d nodes lines in %d device and %d host chunks" %
              (rep["nodes"], rep["reached"], tree.max_depth, rep["nodes_lines"], rep["device_chunks"], rep["host_chunks"]))
        # 2. the taxnodes goal: requested ids with their descendants down to the species level, without the excluded subtrees
        requested, excluded = host.read_taxids_file(taxids_path)
        selected = tree.select(tree.nodes_of(requested, a["taxids"]), tree.nodes_of(excluded, a["taxids"]), "species")
        print("taxnodes: " + ", ".join(str(t) for t in a["taxids"][selected > 0]))
        # 3. the accession map over the tree's ids: a node of the map is a node of the tree
        amap, _ = host.accmap_files([catalog_path], a["taxids"], CATEGORIES, STATUSES, "GENOMIC")
        _, _, regions = amap.fetch()
        # 4. the tree the database carries: the selected nodes that have regions, and their ancestors
        flagged = np.where(selected > 0, regions, 0).astype(np.int32)
        small = tree.small_tree(flagged)
        vi_of_node = np.full(tree.n_nodes, -1, dtype=np.int32)
        vi_of_node[small["node_of_vi"]] = np.arange(len(small["node_of_vi"]), dtype=np.int32)
        print("small tree: " + ", ".join(f"{a['taxids'][n]} <- {a['taxids'][small['node_of_vi'][p]] if p >= 0 else '-'}"
                                         for n, p in zip(small["node_of_vi"], small["parent_vi"])))
        # 5. the store: every record is looked up on the device; a record counts under the nearest selected ancestor of its node --
        #    here simply the node itself if it is selected (E. coli K-12 lies below the species cut and is left out)
        builder = ga.DeviceDbBuilder(31, len(small["parent_vi"]), small["parent_vi"])

        def resolve(_file, _first, node):
            return np.where((node >= 0) & (selected[np.maximum(node, 0)] > 0), vi_of_node[np.maximum(node, 0)], -1).astype(np.int32)

        for update in (False, True):
            host.genome_files_mapped(fasta_paths, amap, resolve, lambda seq, off, vi: builder.add(seq, off, vi, update=update), complete_only=True)
        kmers, value_idx = builder.finish()
        builder.close()
        amap.close()
        print("store: %d k-mers under %d values" % (len(kmers), len(small["parent_vi"])))
        # 6. a match; the table's rows carry names and ranks from the tree
        store = ga.DeviceKMerStore(31, kmers, value_idx, len(small["parent_vi"]), small["parent_vi"])
        matcher = ga.FastqKMerMatcher(store)
        seq = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
        matcher.match_reads(seq, off)
        table, _ = matcher.finish()
        print("taxid;name;rank;reads;kmers")
        for vi, node in enumerate(small["node_of_vi"]):
            rank = ga.RANK_NAMES[a["rank"][node]] if a["rank"][node] >= 0 else ""
            print("%d;%s;%s;%d;%d" % (a["taxids"][node], (names[node] or b"").decode(), rank, table[vi][0], table[vi][2]))
        tree.close()


if __name__ == "__main__":
    main()
