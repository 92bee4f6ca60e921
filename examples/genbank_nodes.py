"""Which nodes of a build are short of RefSeq genomes: nodes.dmp / names.dmp -> the tree, taxids.txt -> the taxnodes set, a RefSeq
catalog -> the accession map and its regions per node -> the count of every node with everything below it -> the selected nodes
whose count is below refSeq.limitForGenbankAccess (the taxfromgenbank goal).

    python examples/genbank_nodes.py --demo

writes a small dump, a tax id file and a catalog in which three of five species are short of genomes, and names them.
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host  # noqa: E402

# id, parent, rank, name
TAXA = [(1, 1, "no rank", "root"), (2, 1, "superkingdom", "Bacteria"), (561, 2, "genus", "Escherichia"), (562, 561, "species", "Escherichia coli"),
        (83333, 562, "strain", "Escherichia coli K-12"), (511145, 83333, "no rank", "Escherichia coli str. K-12 substr. MG1655"),
        (564, 561, "species", "Escherichia fergusonii"), (208962, 561, "species", "Escherichia albertii"),
        (1279, 2, "genus", "Staphylococcus"), (1280, 1279, "species", "Staphylococcus aureus"), (1282, 1279, "species", "Staphylococcus epidermidis")]
# E. coli has its genomes at a strain and a substrain below it, none at the species itself; E. fergusonii has one; E. albertii
# none; S. aureus three; S. epidermidis one
CATALOG = [("NC_000913.3", 511145), ("NZ_000001.1", 511145), ("NZ_000002.1", 83333), ("NC_011740.1", 564), ("NC_007795.1", 1280), ("NZ_000003.1", 1280),
           ("NZ_000004.1", 1280), ("NZ_000005.1", 1282)]
LIMIT = 2  # refSeq.limitForGenbankAccess: a species with fewer entries than this is looked up in Genbank


def write_demo(tmp):
    p = lambda name: os.path.join(tmp, name)
    open(p("nodes.dmp"), "w").write("".join(f"{t}\t|\t{par}\t|\t{rank}\t|\t\t|\t0\t|\t1\t|\t11\t|\n" for t, par, rank, _ in TAXA))
    open(p("names.dmp"), "w").write("".join(f"{t}\t|\t{name}\t|\t\t|\tscientific name\t|\n" for t, _, _, name in TAXA))
    open(p("taxids.txt"), "w").write("# the demo's request\n2\n")
    open(p("catalog"), "w").write("".join(f"{t}\tSome name\t{acc}\tcomplete|bacteria\tREVIEWED\t5000\n" for acc, t in CATALOG))
    return p("nodes.dmp"), p("names.dmp"), p("taxids.txt"), p("catalog")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--demo", action="store_true")
    if not ap.parse_args().demo:
        ap.error("give --demo")
    with tempfile.TemporaryDirectory() as tmp:
        nodes_path, names_path, taxids_path, catalog_path = write_demo(tmp)
        # 1. the tree, and 2. the taxnodes set down to the species level
        tree, _ = host.taxtree_files(nodes_path, names_path)
        a, names = tree.arrays(), tree.names()
        requested, excluded = host.read_taxids_file(taxids_path)
        selected = tree.select(tree.nodes_of(requested, a["taxids"]), tree.nodes_of(excluded, a["taxids"]), "species")
        # 3. the accession map over the tree's ids; its regions count the entries of every node itself
        amap, _ = host.accmap_files([catalog_path], a["taxids"], ["bacteria"], ["REVIEWED"], "GENOMIC")
        _, _, regions = amap.fetch()
        amap.close()
        # 4. the count the reference keeps -- an entry counts for its node and for every ancestor -- and the species below the limit
        below, inclusive = tree.regions_below(regions, selected, LIMIT, "species")
        print("taxid;name;rank;entries at the node;entries with everything below it")
        for node in range(tree.n_nodes):
            if selected[node]:
                rank = ga.RANK_NAMES[a["rank"][node]] if a["rank"][node] >= 0 else ""
                print("%d;%s;%s;%d;%d" % (a["taxids"][node], (names[node] or b"").decode(), rank, regions[node], inclusive[node]))
        print("short of RefSeq genomes (fewer than %d entries): %s" % (LIMIT, ", ".join("%d %s" % (a["taxids"][v], names[v].decode()) for v in below)))
        short = sorted(int(a["taxids"][v]) for v in below)
        assert short == [564, 1282, 208962], short  # E. coli is not among them: its three entries lie below the species
        tree.close()


if __name__ == "__main__":
    main()
