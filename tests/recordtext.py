"""Helpers of the tests of the per-read outputs of FASTA and general FASTQ chunks (tests/test_gpu_record_text.py,
tests/test_gpu_record_files.py): builders of such text, and the expected record text / Kraken-style lines from
streamgoals.read_entries and krakenlines.line.  A helper module of the suite, not a test file; nothing here calls the library
except Side, which holds a store on the device next to the same store in the oracle."""
import numpy as np

import krakenlines
import matchcheck
import streamgoals
from oracle import gs_oracle as orc


def wrap(s, n_lines):
    """s cut into n_lines lines (the last ones may be short, none is empty while bytes are left)"""
    s = bytes(s)
    per = max(1, -(-len(s) // n_lines))
    parts = [s[i:i + per] for i in range(0, len(s), per)] or [b""]
    return parts


def fasta(recs, width=60, crlf=False):
    """[(header line with its '>', sequence)] -> FASTA text, the sequence over lines of `width`; an empty sequence: no line"""
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for d, s in recs:
        out.append(bytes(d) + nl)
        out.extend(bytes(s[i:i + width]) + nl for i in range(0, len(s), width))
    return b"".join(out)


def fastq_ml(recs, crlf=False):
    """[(descriptor line, sequence, quality, sequence lines, quality lines)] -> general FASTQ text.  A quality longer than the
    sequence overshoots in its LAST line: the lines in front of it hold less than the sequence needs."""
    nl = b"\r\n" if crlf else b"\n"
    out = []
    e = len(nl) - 1  # (a '\r' counts into the length of its line, for the sequence and for the qualities)
    for d, s, q, n_seq, n_qual in recs:
        sparts = wrap(s, n_seq)
        need = len(s) + len(sparts) * e  # the reader stops as soon as the quality lines hold this many characters
        body = q[:max(0, min(len(s) - 1, need - 1 - (n_qual - 1) * e))] if n_qual > 1 else b""
        qparts = (wrap(body, n_qual - 1) if body else []) + [q[len(body):]]
        assert len(s) > 0 and len(q) + len(qparts) * e >= need and len(body) + (len(qparts) - 1) * e < need
        out.append(bytes(d) + nl + nl.join(sparts) + nl + b"+" + nl + nl.join(qparts) + nl)
    return b"".join(out)


def entries(data, is_fasta):
    """streamgoals.read_entries as a list: (descriptor, read, quality or None) per record"""
    return list(streamgoals.read_entries(data, is_fasta))


def record_text(ents, keep, with_probs):
    """ReadEntry.write of the entries whose keep flag is set"""
    out = bytearray()
    for (d, r, q), k in zip(ents, keep):
        if k:
            out += d + b"\n" + r + b"\n+\n" + (q if q is not None and with_probs else b"~" * len(r)) + b"\n"
    return bytes(out)


def kraken_text(ents, k, segments, class_vi, taxids, write_all=True):
    """the Kraken-style lines of the entries, one per read that prints one"""
    assert len(ents) == len(class_vi)
    return b"".join(krakenlines.line(d, len(r), k, segments(r) if len(r) >= k else [], int(c), taxids, write_all) for (d, r, _), c in zip(ents, class_vi))


class Side:
    """a store on the device, the same store in the oracle, and the oracle's segments per distinct read"""

    def __init__(self, ga, k, kmers, vidx, n_values, parent):
        self.k = k
        self.store = ga.DeviceKMerStore(k, kmers, vidx, n_values, parent)
        self.odb = orc.DB(k, kmers, vidx, n_values, parent)
        self._segs = {}

    def segments(self, read):
        read = bytes(read)
        if read not in self._segs:
            self._segs[read] = self.odb.segments(read, cap=max(4096, len(read) + 1))
        return self._segs[read]

    def match(self, reads, **cfg):
        """(class_vi, flags) of the oracle for these reads"""
        if not reads:
            return np.zeros(0, np.int32), np.zeros(0, np.uint8)
        seq, off = orc.pack_reads([bytes(r) for r in reads])
        o = matchcheck.oracle_batch(self.odb, seq, off, **cfg)
        return o["class_vi"], o["flags"]

    def close(self):
        self.store.close()
