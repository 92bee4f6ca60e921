"""The accmapsize / accmap goals and the header lookup in plain Python, as the reference does them (see
genestrip_amd/csrc/gs_accmapparse.h for the sources): one 2048-byte line buffer that lives across the lines of a stream, NUL bytes
dropped, fields found by five indexOf calls that restart at 0 behind a miss, an entry that passes on prefix, category and status
and is put if its tax id field names a node.  Not used by the product; the tests hold the device and the C++ parser to it."""

MAX_LINE = 2048
DNA = (b"AC_", b"NC_", b"NG_", b"NT_", b"NW_", b"NZ_")
RNA = (b"NR_", b"XR_")
MRNA = (b"NM_", b"XM_")
COMPLETE = (b"AC_", b"NC_", b"NZ_", b"NM_", b"XM_", b"NR_", b"XR_")
SEQ_TYPES = {"GENOMIC": (1, 0, 0), "RNA": (0, 1, 0), "M_RNA": (0, 0, 1), "ALL_RNA": (0, 1, 1), "ALL": (1, 1, 1)}


class Throws(Exception):
    """the reference throws; .line: the 1-based line"""

    def __init__(self, line, why):
        super().__init__(f"line {line}: {why}")
        self.line = line


def _index_of(target, start, end, pat):
    """ByteArrayUtil.indexOf(array, start, end, char / String): the match lies inside [start, end)"""
    if end - len(pat) < start:
        return -1
    return target.find(pat, start, end)


def _node_of(field, known_index):
    """DigitTrie.get over the canonical decimal strings: None on a non-digit, on '007', on an empty field"""
    if not field or not field.isdigit() or field[0:1] == b"0" or len(field) > 10:
        return None
    return known_index.get(int(field))


def process_catalog(data, seq_type, categories, statuses, known_taxids):
    """one stream -> (passing, [(key bytes, node)] in input order, lines); raises Throws where the reference throws"""
    dna, rna, mrna = SEQ_TYPES[seq_type] if isinstance(seq_type, str) else seq_type
    prefixes = (DNA if dna else ()) + (RNA if rna else ()) + (MRNA if mrna else ())
    cats = [c.encode() if isinstance(c, str) else bytes(c) for c in categories]
    stats = [s.encode() if isinstance(s, str) else bytes(s) for s in statuses]
    known_index = {int(t): i for i, t in enumerate(known_taxids)}
    target = bytearray(MAX_LINE)
    passing, entries, lines = 0, [], 0
    pos = 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        stop = len(data) if nl < 0 else nl + 1
        size, c = 0, -1
        line = data[pos:stop]
        if len(line) <= MAX_LINE and 0 not in line:  # (the loop below, in one step)
            size, c = len(line), line[-1]
            target[:size] = line
            line = b""
        for c in line:  # BufferedLineReader.nextLine
            if size == MAX_LINE:
                raise Throws(lines + 1, "line does not fit the buffer")
            target[size] = c
            if c != 0:
                size += 1
        if c != 10 and size == MAX_LINE:
            raise Throws(lines + 1, "line does not fit the buffer")
        pos = stop
        if size == 0:
            break
        lines += 1
        pos1 = _index_of(target, 0, size, b"\t")
        pos2 = _index_of(target, pos1 + 1, size, b"\t")
        pos3 = _index_of(target, pos2 + 1, size, b"\t")
        pos4 = _index_of(target, pos3 + 1, size, b"\t")
        pos5 = _index_of(target, pos4 + 1, size, b"\t")
        if pos2 + 1 + 3 > MAX_LINE or bytes(target[pos2 + 1:pos2 + 4]) not in prefixes:  # (startsWith reads stale bytes behind the line)
            continue
        if not any(_index_of(target, pos3 + 1, pos4, c) >= 0 for c in cats):
            continue
        if not any(_index_of(target, pos4 + 1, pos5, s) >= 0 for s in stats):
            continue
        passing += 1
        node = _node_of(bytes(target[0:pos1]) if pos1 > 0 else b"", known_index)
        if node is None:
            continue
        if pos3 < pos2 + 1:
            raise Throws(lines, "put with a negative length")
        entries.append((bytes(target[pos2 + 1:pos3]), node))
    return passing, entries, lines


def key_order(key):
    """AccessionMapImpl.compareBytes: length, then signed bytes"""
    return (len(key), [b - 256 if b >= 128 else b for b in key])


def finish(entries):
    """-> (sorted entries, ties in input order; duplicates; conflicts)"""
    s = sorted(entries, key=lambda e: key_order(e[0]))
    dup = sum(1 for a, b in zip(s, s[1:]) if a[0] == b[0])
    conflicts = sum(1 for a, b in zip(s, s[1:]) if a[0] == b[0] and a[1] != b[1])
    return s, dup, conflicts


def first_nodes(entries):
    """{key: node of its first entry in input order}: what a lookup answers with among equal keys"""
    d = {}
    for k, node in entries:
        d.setdefault(k, node)
    return d


def lookup(first, header, complete_only=False):
    """updateNodeFromInfoLine over AccessionMapImpl.get, `first` from first_nodes().  -1: no node"""
    blank = header.find(b" ")
    if blank < 1:
        return -1
    key = header[1:blank]
    if complete_only and key[:3] not in COMPLETE:
        return -1
    return first.get(key, -1)


def in_grammar(line, seq_type, categories, statuses, terminated=True):
    """is this line (with its newline, if it has one) inside the device's grammar (gs_accmap.hip)"""
    if line == b"\n":
        return True
    if b"\0" in line:
        return False
    if len(line) > MAX_LINE or (not line.endswith(b"\n") and len(line) >= MAX_LINE):
        return False
    f = line.rstrip(b"\n").split(b"\t") if line.endswith(b"\n") else line.split(b"\t")
    if len(f) < 6:
        return False
    passing, _, _ = process_catalog(line, seq_type, categories, statuses, [])
    if not passing:
        return True
    tax, acc = f[0], f[2]
    return 1 <= len(tax) <= 9 and tax.isdigit() and tax[0:1] != b"0" and len(acc) <= 31 and all(b < 0x80 for b in acc)
