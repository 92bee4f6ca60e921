"""The Kraken-style output line of a read (FastqKMerMatcher.java:308-314, :597-611, MatcherReadEntry.writeMatchDetails :723-756),
restated in plain Python from the oracle's segments and a class array.  A helper module of the suite, not a test file, and
independent of the library: nothing here calls it.

Reads are 0-based in a chunk of four-line records, nl = the byte offsets of the chunk's newlines:
  descriptor line = text[d0:d1] with d0 = nl[4r-1] + 1 (0 for r = 0), d1 = nl[4r]
  L = nl[4r+1] - d1 - 1 (a '\\r' in front of the newline counts), max = L - k + 1
No line if the read has no segment (max <= 0) or not (write_all or class >= 0).  Otherwise
  'C' | 'U'  TAB  name  TAB  taxids[class] | '0'  TAB  L  TAB  segments joined by single blanks  NL
name = the descriptor bytes from index 1 up to the first blank at an index >= 1 (all of them if there is none, nothing if the
descriptor has at most one byte), copied as they are.  A segment is taxids[code] | '0' (code -1) | 'A' (code -2), ':' and its count
of positions.
"""
import numpy as np


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def name_of(desc):
    """the printed name of a descriptor line (bytes, its first byte -- the '@' -- included)"""
    desc = bytes(desc)
    if len(desc) <= 1:
        return b""
    i = desc.find(b" ", 1)
    return desc[1:] if i < 0 else desc[1:i]


def records(text):
    """(descriptor line, sequence line) of every record of a four-line chunk, cut at the newline offsets as the rule above says"""
    text = bytes(text)
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
    assert len(nl) % 4 == 0, "whole four-line records"
    out = []
    for r in range(len(nl) // 4):
        d0 = int(nl[4 * r - 1]) + 1 if r else 0
        d1 = int(nl[4 * r])
        out.append((text[d0:d1], text[d1 + 1:int(nl[4 * r + 1])]))
    return out


def line(desc, L, k, segs, cls, taxids, write_all=True):
    """the line of one read (bytes, newline included) or b"" if it prints none.  segs: [(code, count)] as DB.segments(read) of the
    oracle gives them; cls: the value index of the read's class, < 0 for none; taxids: str or bytes per value index"""
    if L - k + 1 <= 0 or not segs:
        return b""
    if not (write_all or cls >= 0):
        return b""
    assert sum(n for _, n in segs) == L - k + 1, "the counts cover the read's positions"
    tax = lambda v, none: _b(taxids[v]) if v >= 0 else none
    parts = [tax(code, b"A" if code == -2 else b"0") + b":" + str(n).encode() for code, n in segs]
    return (b"C" if cls >= 0 else b"U") + b"\t" + name_of(desc) + b"\t" + tax(cls, b"0") + b"\t" + str(L).encode() + b"\t" + b" ".join(parts) + b"\n"


def chunk_lines(text, k, segments, class_vi, taxids, write_all=True):
    """the lines of a four-line chunk, one entry per read (b"" where a read prints none).  segments: callable read bytes ->
    [(code, count)]; class_vi: per read"""
    recs = records(text)
    assert len(recs) == len(class_vi)
    return [line(d, len(s), k, segments(s) if len(s) >= k else [], int(c), taxids, write_all) for (d, s), c in zip(recs, class_vi)]
