"""The `db2fastq` goal (C/goals/DB2FastqGoal.java): the stored k-mers of a store written as FASTQ, one read per k-mer, as
KMerFastqGenerator + FastQWriter write them.  Taxids as in the reference's `taxids` setting: "X" = the k-mers of tax id X,
"X+" = of X and its subtree, none = one `total` file with every k-mer.  Files are gzip (BGZF) unless --plain
(GSConfigKey gzipFastqOutput, default on).

    python examples/db2fastq.py --store demo.gss --taxids taxids.txt --project myproject 1001 100002+
    python examples/db2fastq.py --demo

--taxids names a text file with the tax id of every value index, one per line (what the host keeps beside a store file:
the .gss image holds no tax id strings).  --demo uses the synthetic store of genestrip_amd.synth and its tax ids.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("select", nargs="*", help='tax ids: "X" (exact) or "X+" (with descendants); none = one "total" file')
    ap.add_argument("--store", help="native store file written by DeviceKMerStore.save()")
    ap.add_argument("--taxids", help="tax id of every value index, one per line")
    ap.add_argument("--demo", action="store_true", help="synthetic store and tax ids")
    ap.add_argument("--project", default="demo")
    ap.add_argument("--out-dir", default=".")
    ap.add_argument("--plain", action="store_true", help="plain text instead of gzip")
    args = ap.parse_args()
    if args.demo:
        db = synth.SynthDB(genome_len=20000)
        store = ga.DeviceKMerStore(31, db.kmers, db.value_idx, db.n_values, db.parent_vi)
        taxids = db.taxids
        select = args.select or ["1001", "100002"]
    else:
        if not (args.store and args.taxids):
            ap.error("give --demo, or --store and --taxids")
        store = ga.DeviceKMerStore.load(args.store)
        taxids = [t.strip() for t in open(args.taxids) if t.strip()]
        select = args.select
    vi_of = {t: v for v, t in enumerate(taxids)}
    jobs = [("total", None, True)] if not select else []
    for s in select:
        desc = s.endswith("+")
        t = s[:-1] if desc else s
        if t not in vi_of:
            ap.error(f"unknown tax id {t}")
        jobs.append((t, vi_of[t], desc))
    suffix = ".fastq" if args.plain else ".fastq.gz"
    for name, vi, desc in jobs:
        path = os.path.join(args.out_dir, f"{args.project}_db2fastq_{name}{suffix}")
        n = host.db2fastq(store, taxids, args.project, path, select=vi, with_desc=desc)
        print(f"{path}: {n} k-mers")
    store.close()


if __name__ == "__main__":
    main()
