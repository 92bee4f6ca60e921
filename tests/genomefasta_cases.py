"""Hand-written genome FASTA streams with the answers worked out from the reference's Java (tests/genomefasta.py names the three
functions).  A helper module, not a test file: tests/test_genomefasta_cpu.py holds the restatement to them, the GPU tests hold the
device and the host parser of include/gshost.h to them as well.

(name, data, last, headers, seq, offsets, max_line, consumed)"""

CASES = [
    # nextLine returns ">a\n" (3), "AC\n" (3), "GT\n" (3), then 0.  dataLine: end steps back over the '\n'.
    ("LF", b">a\nAC\nGT\n", True, [b">a"], b"ACGT", [0, 4], 3, 9),
    # "AC\r\n": size 4; the while at :95 steps over '\n' and then over '\r'.  The header line keeps its '\r' (infoLine sees it).
    ("CRLF", b">a\r\nAC\r\nGT\r\n", True, [b">a\r"], b"ACGT", [0, 4], 4, 12),
    # "AC\r\r\n": the while steps over all three terminators
    ("two CR", b">a\nAC\r\r\n", True, [b">a"], b"AC", [0, 2], 5, 8),
    # "A\rC\n": the while stops at 'C'; the '\r' in front of it is put like any byte (it resets the k-mer window later)
    ("CR inside a line", b">a\nA\rC\n", True, [b">a"], b"A\rC", [0, 3], 4, 7),
    ("CR run inside a line", b">a\nA\r\rC\r\n", True, [b">a"], b"A\r\rC", [0, 4], 6, 9),
    # "\n": size 1 > 0, so the loop goes on; target[0] is '\n', a data line; end steps back to 0: nothing is put.  "\r\n" alike.
    ("empty lines", b">a\nAC\n\nGT\n\r\n", True, [b">a"], b"ACGT", [0, 4], 3, 12),
    ("a line of one CR", b">a\n\r\nAC\n", True, [b">a"], b"AC", [0, 2], 3, 8),
    # a header line right behind a header line: endRegion, startRegion -- a region without bases
    ("header-only records", b">a\n>b\nAC\n>c\n", True, [b">a", b">b", b">c"], b"AC", [0, 0, 2, 2], 3, 12),
    # `first` is still true at "ACGT\n": no region is open (includeRegion is false until an infoLine sets it)
    ("data in front of the first header", b"ACGT\n\n>a\nGG\n", True, [b">a"], b"GG", [0, 2], 5, 12),
    # the last nextLine returns "GT" (2) when the stream ends; the while finds no terminator
    ("no final newline", b">a\nAC\nGT", True, [b">a"], b"ACGT", [0, 4], 3, 8),
    # ... and "GT\r" (3): :95 asks for '\n' OR '\r', so the bare '\r' at the end of the stream IS stripped
    ("final bare CR", b">a\nAC\nGT\r", True, [b">a"], b"ACGT", [0, 4], 3, 9),
    ("final header without newline", b">a\nAC\n>b", True, [b">a", b">b"], b"AC", [0, 2, 2], 3, 8),
    # only target[0] is compared with '>'
    ("'>' inside a data line", b">a\nAC>GT\n", True, [b">a"], b"AC>GT", [0, 5], 6, 9),
    ("lower case stays", b">a\nacgtN\n", True, [b">a"], b"acgtN", [0, 5], 6, 9),
    # nextLine does not advance `size` for a NUL: the line is "AC\n" to everything behind it
    ("NUL byte", b">a\nA\x00C\n", True, [b">a"], b"AC", [0, 2], 3, 7),
    ("empty stream", b"", True, [], b"", [0], 0, 0),
    # ---- chunks of a longer stream (last = False): only the records a later header line ends
    ("cut behind a newline", b">a\nAC\n>b\nGG\n", False, [b">a"], b"AC", [0, 2], 3, 6),
    ("cut inside a header line", b">a\nAC\n>b", False, [b">a"], b"AC", [0, 2], 3, 6),
    ("cut inside a data line", b">a\nAC\n\n>b x\nGG\nT", False, [b">a"], b"AC", [0, 2], 3, 7),
    ("one header only", b">a\nAC\n", False, [], b"", [0], 0, 0),
    ("no header at all", b"AC\nGT", False, [], b"", [0], 3, 3),
    ("no header, no newline", b"ACGT", False, [], b"", [0], 0, 0),
]
