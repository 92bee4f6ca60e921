"""The `krakencount` / `krakenres` goals (C/goals/kraken/KrakenResCountGoal.java, KrakenResFileGoal.java): per tax id of
Kraken-style output files -- this project's, Kraken's, KrakenUniq's; plain or gzip -- the reads, the k-mers and the k-mers in
matching reads, printed as the reference's CSV.  The lines are counted on the device.

    python examples/kraken_count.py sample1.kraken.out.gz sample2.kraken.out
    python examples/kraken_count.py --demo

--demo matches synthetic reads against a synthetic store with the Kraken-style lines written on the device into a .gz, counts
that file, and checks the counts against the match run's own table: for every tax id of the store, the k-mers of its segments are
the table's "kmers" column and the lines of its class are the table's "reads" column.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host, synth  # noqa: E402


def demo(tmp):
    db = synth.SynthDB(k=31, genera=2, species_per_genus=3, genome_len=20000, seed=3)
    seq, off = synth.reads_host(db.genomes, 20000, read_len=150, seed=77)
    rng = np.random.default_rng(1)
    fq = os.path.join(tmp, "reads.fastq")
    with open(fq, "wb") as f:
        for i in range(len(off) - 1):
            r = bytes(seq[int(off[i]):int(off[i + 1])])
            if i % 4 == 0:
                r = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 150))  # background
            if i % 9 == 0:
                r = r[:60] + b"NNN" + r[63:]
            f.write(b"@read%d:%d\n" % (i, i % 7) + r + b"\n+\n" + b"I" * len(r) + b"\n")
    store = ga.DeviceKMerStore(31, db.kmers, db.value_idx, db.n_values, db.parent_vi)
    out = os.path.join(tmp, "reads.kraken.out.gz")
    table, _, _ = host.match_files(store, [fq], kraken_out_path=out, taxids=db.taxids, write_all=True)
    return out, table, db.taxids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*")
    ap.add_argument("--only", help="comma-separated tax ids to keep")
    ap.add_argument("--csv", help="also write the CSV here (.gz: gzip)")
    ap.add_argument("--demo", action="store_true")
    args = ap.parse_args()
    table = taxids = None
    if args.demo:
        out, table, taxids = demo(tempfile.mkdtemp())
        files = [out]
    elif args.files:
        files = args.files
    else:
        ap.error("give --demo or input files")
    rows, tot = host.kraken_count_files(files, only=args.only.split(",") if args.only else None, csv=args.csv)
    print("taxid;reads;kmers;kmers in matching reads")
    for key, reads, kmers, kimr in rows:
        print(f"{key.decode(errors='replace')};{reads};{kmers};{kimr};")
    print(f"# {tot['lines']} lines, {tot['counted_tokens']} tokens counted, {tot['a_tokens']} 'A' tokens skipped, {tot['long_lines']} long lines; "
          f"{tot['device_chunks']} chunks on the device, {tot['host_chunks']} line by line; {tot['seconds_total'] * 1e3:.1f} ms", file=sys.stderr)
    if args.demo:
        by_key = {k.decode(): (r, km) for k, r, km, _ in rows}
        bad = 0
        for vi, t in enumerate(taxids):
            reads, kmers = by_key.get(t, (0, 0))
            ok = kmers == int(table[vi, 2]) and reads == int(table[vi, 0])
            bad += not ok
            print(f"# tax id {t}: kmers {kmers} / table {int(table[vi, 2])}, reads {reads} / table {int(table[vi, 0])}: {'match' if ok else 'DIFFER'}")
        print("# identities hold" if not bad else f"# {bad} tax ids DIFFER")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
