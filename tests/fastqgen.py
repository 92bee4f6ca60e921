"""The reference's db2fastq text restated in Python: KMerFastqGenerator.generateFastq (C/fastqgen/KMerFastqGenerator.java) over
FastQWriter (C/fastqgen/FastQWriter.java), and the k-mer selection of DB2FastqGoal.  A helper module of the suite, not a test file.
"""
import numpy as np

GENESTRIP_ID = "@GENESTRIP"
DECODE = "CGAT"  # CGAT.DECODE_TABLE


def kmer_straight(kmer, k):
    """CGAT.longToKMerStraight: first base in the top bits"""
    return "".join(DECODE[(int(kmer) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def fastq_text(kmers, value_idx, taxids, k, project):
    """FastQWriter(GENESTRIP_ID + ":" + header) with header = project + ":", addRead(node.getTaxId(), bases) per k-mer in visit
    order: `added` is incremented before the descriptor is printed, so reads count from 1"""
    ident = GENESTRIP_ID + ":" + project + ":"
    out = []
    for n, (x, v) in enumerate(zip(kmers, value_idx), start=1):
        out.append(f"{ident}:{taxids[int(v)]}:{n}\n{kmer_straight(x, k)}\n+\n{'~' * k}\n")
    return "".join(out).encode()


def subtree(parent_vi, v):
    """bool[n_values]: the values whose node has v on its path to the root (v included) -- isMatchingNode with withDesc"""
    parent_vi = np.asarray(parent_vi)
    out = np.zeros(len(parent_vi), dtype=bool)
    for u in range(len(parent_vi)):
        w = u
        while w >= 0:
            if w == v:
                out[u] = True
                break
            w = int(parent_vi[w])
    return out


def revcomp(x, k):
    """the reverse complement in the reference encoding (complement = code ^ 1)"""
    r = 0
    for i in range(k):
        r = (r << 2) | (((int(x) >> (2 * i)) & 3) ^ 1)
    return r


def revcomp_np(x, k):
    """revcomp over a numpy array (uint64 bit tricks: complement the low code bits, reverse the 2-bit groups)"""
    x = np.asarray(x).astype(np.uint64) ^ np.uint64(((1 << (2 * k)) - 1) & 0x5555555555555555)
    for sh, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        m = np.uint64(m)
        x = ((x >> np.uint64(sh)) & m) | ((x & m) << np.uint64(sh))
    x = (x >> np.uint64(32)) | (x << np.uint64(32))
    return (x >> np.uint64(64 - 2 * k)).astype(np.int64)


def stored_pairs(kmers, value_idx, parent_vi, k):
    """the contract of the export: the input pairs that are reachable (x >= revcomp(x)) and whose value has a tree node, ascending"""
    kmers = np.asarray(kmers, dtype=np.int64)
    value_idx = np.asarray(value_idx, dtype=np.int32)
    keep = kmers >= revcomp_np(kmers, k)
    if parent_vi is not None:
        keep &= np.asarray(parent_vi)[value_idx] != -2
    o = np.argsort(kmers[keep], kind="stable")
    return kmers[keep][o], value_idx[keep][o]
