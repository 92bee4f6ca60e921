"""The `fasta2fastq` goal (C/goals/Fasta2FastqGoal.java): FASTA records -- an assembly, a genome -- rewritten as four-line
FASTQ with '~' qualities, so that they can be matched like reads.  All inputs (plain, gzip or BGZF) go into ONE output, in order;
the text is made on the device.  The output is gzip (BGZF) when its name ends in .gz.

    python examples/fasta2fastq.py --out assembly.fastq.gz contigs1.fasta contigs2.fasta.gz
    python examples/fasta2fastq.py --demo
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
    ap.add_argument("--out", help="FASTQ file to write (.gz: gzip)")
    ap.add_argument("--demo", action="store_true", help="a small assembly of its own")
    args = ap.parse_args()
    if args.demo:
        tmp = tempfile.mkdtemp()
        src = os.path.join(tmp, "contigs.fasta")
        with open(src, "wb") as f:
            for i in range(2000):
                f.write(b">contig_%d len=%d\n" % (i, 60 * (1 + i % 50)) + (b"ACGTTGCA" * 7 + b"ACGT\n") * (1 + i % 50))
        files, out = [src], os.path.join(tmp, "contigs.fastq.gz")
    else:
        if not (args.files and args.out):
            ap.error("give --demo, or --out and input files")
        files, out = args.files, args.out
    n = host.fasta2fastq(files, out)
    print(f"{out}: {n} records")
    if args.demo:
        text = gzip.open(out).read()
        assert n == 2000 and text.count(b"\n+\n") == 2000 and text.startswith(b"@contig_0 len=60\n" + b"ACGTTGCA" * 7 + b"ACGT\n+\n" + b"~" * 60)


if __name__ == "__main__":
    main()
