"""From the nodes that are short of RefSeq genomes to a store that holds their Genbank genomes: examples/genbank_nodes.py ends with
the taxfromgenbank set; this goes on with the Genbank assembly summary -> the entries of those nodes that pass quality and
reference rules -> the best genbank.maxPerTaxid of each node and their file names (the fastasgenbank goal)
-> the FASTA files under those names -> regions -> a store -> a read from a Genbank-only genome classified to its node.

    python examples/genbank_fastas.py --demo

The summary is judged on the device chunk by chunk; a chunk outside the device's grammar (a CR, a non-ASCII key) goes through the
record-by-record restatement of the reference inside the same call.  Downloading is not part of this: the demo writes the genomes.
"""
import argparse
import gzip
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host  # noqa: E402
from genbank_nodes import LIMIT, TAXA, write_demo  # noqa: E402

FTP = "https://ftp.ncbi.nlm.nih.gov/genomes/all/GCA"
# accession, assembly name, refseq category, tax id, species tax id, version status, assembly level, submitter
ASSEMBLIES = [
    ("GCA_000026225.1", "ASM2622v1", "na", 564, 564, "latest", "Scaffold", "Genoscope"),                         # quality not allowed
    ("GCA_000026226.1", "ASM2623v1", "representative genome", 585054, 564, "latest", "Complete Genome", "Génoscope"),  # a strain: no node
    ("GCA_000026227.2", "ASM2624v2", "na", 564, 564, "latest", "Complete Genome", "Génoscope"),
    ("GCA_000026228.1", "ASM2625v1", "na", 564, 564, "latest", "Chromosome", "Universität Würzburg"),            # the cap drops it
    ("GCA_001281005.1", "ASM128100v1", "na", 1282, 1282, "latest", "Chromosome", "NIH"),
    ("GCA_001281006.1", "ASM128101v1", "na", 1282, 1282, "replaced", "Complete Genome", "NIH"),                   # not latest
    ("GCA_002895205.1", "ASM289520v1", "reference genome", 208962, 208962, "latest", "Complete Genome", "FDA"),
    ("GCA_002895206.1", "ASM289521v1", "na", 208962, 208962, "latest", "Complete Genome", "FDA"),                 # equal quality, later: it stays
    ("GCA_000005845.2", "ASM584v2", "reference genome", 511145, 562, "latest", "Complete Genome", "Univ. Wisconsin"),  # E. coli has RefSeq genomes
]


def summary_text():
    rows = ["## See ftp://ftp.ncbi.nlm.nih.gov/genomes/README_assembly_summary.txt for a description of the columns in this file.",
            "#assembly_accession\tbioproject\tbiosample\twgs_master\trefseq_category\ttaxid\tspecies_taxid\torganism_name"]
    for acc, asm, cat, taxid, species, status, level, submitter in ASSEMBLIES:
        f = [acc, "PRJNA1", "SAMN1", "", cat, str(taxid), str(species), "Some organism", "strain=x", "", status, level, "Major", "Full", "2020/01/01", asm,
             submitter, "na", "", "%s/%s/%s/%s/%s_%s" % (FTP, acc[4:7], acc[7:10], acc[10:13], acc, asm), "", "na", "na", "haploid", "bacteria",
             "5000000", "4900000", "50.5", "1", "1", "1", "na", "na", "na", "na", "na", "na", "na"]
        rows.append("\t".join(f))
    return ("\n".join(rows) + "\n").encode("utf-8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--demo", action="store_true")
    if not ap.parse_args().demo:
        ap.error("give --demo")
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as tmp:
        # 1. what examples/genbank_nodes.py does: tree, taxnodes set, accession map, the nodes below the limit
        nodes_path, names_path, taxids_path, catalog_path = write_demo(tmp)
        tree, _ = host.taxtree_files(nodes_path, names_path)
        a, names = tree.arrays(), tree.names()
        taxids = [int(t) for t in a["taxids"]]
        requested, excluded = host.read_taxids_file(taxids_path)
        selected = tree.select(tree.nodes_of(requested, a["taxids"]), tree.nodes_of(excluded, a["taxids"]), "species")
        amap, _ = host.accmap_files([catalog_path], a["taxids"], ["bacteria"], ["REVIEWED"], "GENOMIC")
        _, _, regions = amap.fetch()
        amap.close()
        below, _ = tree.regions_below(regions, selected, LIMIT, "species")
        tree.close()
        print("short of RefSeq genomes: " + ", ".join("%d %s" % (taxids[v], names[v].decode()) for v in below))
        # 2. the assembly summary: the entries of those nodes, the best one of each
        summary_path = os.path.join(tmp, "assembly_summary_genbank.txt")
        open(summary_path, "wb").write(summary_text())
        picks, total, totals = host.assembly_summary_files([summary_path], taxids, selected=below, max_per_taxid=1)
        print("%d records, %d kept, %d picked for %d nodes (%d device and %d host chunks)" %
              (total, totals["kept"], totals["picked"], totals["nodes"], totals["device_chunks"], totals["host_chunks"]))
        paths, node_of_file, genomes = [], [], {}
        for node in sorted(picks):
            for e in picks[node]:
                print("  %d %s: %s %s%s" % (taxids[node], names[node].decode(), e["file_name"].decode(), e["quality"], " (reference)" if e["is_reference"] else ""))
                # 3. the download's stand-in: a genome under the entry's file name
                seq = "".join(rng.choice(list("ACGT"), 30000))
                path = os.path.join(tmp, e["file_name"].decode())
                with gzip.open(path, "wt") as f:
                    f.write(">%s Some organism, whole genome\n" % e["file_name"].decode()[:15] + "".join(seq[i:i + 80] + "\n" for i in range(0, len(seq), 80)))
                paths.append(path)
                node_of_file.append(node)
                genomes[node] = seq
        assert sorted(taxids[n] for n in picks) == [564, 1282, 208962], picks
        assert [picks[n][0]["file_name"] for n in sorted(picks)] == [b"GCA_000026227.2_ASM2624v2_genomic.fna.gz", b"GCA_001281005.1_ASM128100v1_genomic.fna.gz",
                                                                      b"GCA_002895206.1_ASM289521v1_genomic.fna.gz"], picks
        # 4. regions -> store: every record of a file gets the node of the file's pick (the fasta reader of the goal's consumers)
        index = {t: i for i, t in enumerate(taxids)}
        parent_vi = np.array([-1 if t == par else index[par] for t, par, _, _ in sorted(TAXA)], dtype=np.int32)
        b = ga.DeviceDbBuilder(31, len(taxids), parent_vi)
        for update in (False, True):
            host.genome_files(paths, lambda file, _first, headers: [node_of_file[file]] * len(headers), lambda seq, off, nodes: b.add(seq, off, nodes, update=update))
        n_kmers = b.finish_count()
        store = b.to_store()
        b.close()
        # 5. a read from a genome that only Genbank has
        node = index[208962]
        read = np.frombuffer(genomes[node][1000:1150].encode(), dtype=np.uint8)
        m = ga.FastqKMerMatcher(store)
        cv, _ = m.match_reads(read, np.array([0, len(read)], dtype=np.uint64))
        m.finish()
        m.close()
        store.close()
        print("store of %d k-mers; a read of Escherichia albertii's Genbank genome is classified as %d %s" % (n_kmers, taxids[int(cv[0])], names[int(cv[0])].decode()))
        assert int(cv[0]) == node, cv


if __name__ == "__main__":
    main()
