"""The `extract` goal (C/goals/ExtractGoal.java): every read whose descriptor starts with a key -- the sample of a multiplexed
file, the reads of one lane -- copied to a FASTQ file with its qualities.  Inputs are FASTQ or FASTA by suffix, plain, gzip or
BGZF; the selection runs on the device.  The output is gzip (BGZF) when its name ends in .gz.

    python examples/extract_reads.py --key SAMPLE7: --out sample7.fastq.gz run1.fastq.gz run2.fastq.gz
    python examples/extract_reads.py --demo
"""
import argparse
import gzip
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genestrip_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*")
    ap.add_argument("--key", help="the descriptor behind its first character starts with this")
    ap.add_argument("--out", help="FASTQ file to write (.gz: gzip)")
    ap.add_argument("-k", type=int, default=31, help="k-mer size (only for the k-mer total that is reported)")
    ap.add_argument("--demo", action="store_true", help="a small multiplexed file of its own")
    args = ap.parse_args()
    if args.demo:
        tmp = tempfile.mkdtemp()
        src = os.path.join(tmp, "multiplexed.fastq.gz")
        with gzip.open(src, "wb") as f:
            for i in range(30000):
                f.write(b"@sample%d:%d\n%s\n+\n%s\n" % (i % 4, i, b"ACGT" * 25, b"I" * 100))
        files, key, out = [src], "sample2:", os.path.join(tmp, "sample2.fastq.gz")
    else:
        if not (args.files and args.key and args.out):
            ap.error("give --demo, or --key, --out and input files")
        files, key, out = args.files, args.key, args.out
    tot = host.extract_files(key, files, out, k=args.k)
    print(f"{out}: {tot.filtered_reads} of {tot.reads} reads ({tot.bps} bp) start with {key!r}, {tot.seconds_total * 1e3:.1f} ms")
    if args.demo:
        assert tot.filtered_reads == 7500 and gzip.open(out).read().count(b"@sample2:") == 7500


if __name__ == "__main__":
    main()
