"""The accession map of a RefSeq build on the GPU: catalog lines -> sorted (accession, node) map -> node per genome record, the way
the accmapsize / accmap goals and AbstractRefSeqFastaReader.updateNodeFromInfoLine do it on one thread.

    python examples/accession_map.py --demo

writes a small synthetic catalog and two FASTA files, builds the map from the catalog file (host.accmap_files), prints its size,
entries, duplicates and the regions per tax id, then builds a k-mer store from the FASTA files twice -- through
host.genome_files_mapped, where the node of every record is looked up on the device from the header lines the scan left there, and
through host.genome_files with a Python dictionary as resolver -- and checks that the two stores are equal.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host  # noqa: E402

TAXIDS = [1, 562, 1280, 9606]  # node = index; node 0 is the root
CATEGORIES, STATUSES = ["bacteria", "vertebrate_mammalian"], ["REVIEWED", "VALIDATED"]


def write_demo(tmp):
    rng = np.random.default_rng(5)
    records = [("NC_000913.3", 562), ("NZ_CP000001.1", 562), ("NC_007795.1", 1280), ("NC_000001.11", 9606), ("NC_999999.1", None), ("NW_000002.1", 9606)]
    catalog = []
    for acc, tax in records:
        if tax is not None:
            catalog.append(f"{tax}\tSome species\t{acc}\tcomplete|{'bacteria' if tax != 9606 else 'vertebrate_mammalian'}\tREVIEWED\t20000\n")
        catalog.append(f"{tax or 562}\tSome species\tWP_{len(catalog):09d}.1\tbacteria\tPROVISIONAL\t300\n")
    catalog.append("1280\tSome species\tNC_000913.3\tbacteria\tVALIDATED\t20000\n")      # the same accession under another tax id
    catalog.append("4932\tAnother species\tNC_001133.9\tbacteria\tREVIEWED\t230218\n")   # passes, but the tree does not hold 4932
    catalog.append("562\tSome species\tNC_000914.1\tbacteria\tINFERRED\t20000\n")        # another status
    cat_path = os.path.join(tmp, "RefSeq-release.catalog")
    open(cat_path, "w").write("".join(catalog))
    paths = []
    for f in range(2):
        lines = []
        for acc, _ in records[f::2]:
            seq = "".join(rng.choice(list("ACGT"), 20000))
            lines.append(f">{acc} Some species chromosome, complete genome\n" if acc != "NW_000002.1" else f">{acc}\n")  # (one header has no blank)
            lines += [seq[i:i + 60] + "\n" for i in range(0, len(seq), 60)]
        paths.append(os.path.join(tmp, f"genomes{f}.fna"))
        open(paths[-1], "w").write("".join(lines))
    return cat_path, paths


def build_store(paths, walk, k=31):
    """FillDBGoal + DBGoal over the files; walk(paths, add) feeds the regions of one walk to add(seq, offsets, nodes)"""
    parent_vi = np.array([-1] + [0] * (len(TAXIDS) - 1), dtype=np.int32)
    b = ga.DeviceDbBuilder(k, len(TAXIDS), parent_vi)
    for update in (False, True):
        walk(paths, lambda seq, off, nodes: b.add(seq, off, nodes, update=update))
    out = b.finish()
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--demo", action="store_true")
    if not ap.parse_args().demo:
        ap.error("give --demo")
    with tempfile.TemporaryDirectory() as tmp:
        cat_path, paths = write_demo(tmp)
        # the accmapsize goal, then the accmap goal: the catalog file is cut into chunks of whole lines and scanned on the device; a
        # chunk outside the device's grammar goes through the line-by-line restatement of the reference inside the same call
        _, size = host.accmap_files([cat_path], TAXIDS, CATEGORIES, STATUSES, "GENOMIC", count_only=True)
        amap, totals = host.accmap_files([cat_path], TAXIDS, CATEGORIES, STATUSES, "GENOMIC", reserve_entries=size["passing"])
        info = (amap.n_entries, amap.n_passing)
        slots, nodes, regions = amap.fetch()
        dup = sum(1 for a, b in zip(slots[1:], slots[:-1]) if bytes(a) == bytes(b))
        print("accmapsize: %d; entries %d, %d of them repeat an accession; %d lines in %d device and %d host chunks" %
              (size["passing"], info[0], dup, totals["lines"], totals["device_chunks"], totals["host_chunks"]))
        print("regions per tax id: " + ", ".join(f"{t}: {r}" for t, r in zip(TAXIDS, regions)))
        first = {}
        for key, node in zip(ga.slot_accessions(slots), nodes):  # (equal keys stand in input order)
            first.setdefault(key, int(node))

        complete = (b"AC_", b"NC_", b"NZ_", b"NM_", b"XM_", b"NR_", b"XR_")  # (completeGenomesOnly)

        def by_dictionary(_file, _first_record, headers):
            keys = [h[1:h.find(b" ")] if b" " in h else None for h in headers]
            return [first.get(k, -1) if k is not None and k[:3] in complete else -1 for k in keys]

        # the device looks the header lines of a chunk up where its scan left them: the resolver sees one node per record
        kmers_d, vidx_d = build_store(paths, lambda p, add: host.genome_files_mapped(p, amap, lambda _f, _r, nodes: nodes, add, complete_only=True))
        kmers_h, vidx_h = build_store(paths, lambda p, add: host.genome_files(p, by_dictionary, add))
        amap.close()
        if not (np.array_equal(kmers_d, kmers_h) and np.array_equal(vidx_d, vidx_h)):
            raise SystemExit("the store built through the device lookup differs from the one built through the dictionary")
        per = np.bincount(vidx_d, minlength=len(TAXIDS))
        print("store: %d k-mers, equal for both resolvers; per tax id: %s" % (len(kmers_d), ", ".join(f"{t}: {n}" for t, n in zip(TAXIDS, per))))


if __name__ == "__main__":
    main()
