"""The krakencount goal in plain Python: KrakenResultProcessor.process (KrakenResultProcessor.java:74-179) under the listener of
KrakenResCountGoal (KrakenResCountGoal.java:133-157), over the lines of BufferedLineReader.nextLine (BufferedLineReader.java
:160-182).  A helper module of the suite, not a test file, and independent of the library: nothing here calls it.

Per stream: NUL bytes are dropped, '\\r' is kept; a line is what nextLine returns without its last byte (the newline -- or, for an
unterminated tail, the tail's last byte); the loop ENDS at the first line that is then empty.  Per line the reference's state
machine is restated as it stands: the first four tabs end flag, descriptor, class and read size; any ':' arms `fr` (never disarmed
inside a line) and sets the count's start; a blank while `fr` is set, or the end of the line, closes a token.  A token whose first
byte is 'A' is skipped, one whose tax id holds a non-digit too (the caught IllegalStateException of DigitTrie.get); a non-digit in
a count, in the read size or in the class fails the call.  Numbers are Java ints (they wrap).  Keys are byte strings.  The class
of a line lives on until the next line's third tab; before the first class it is null, and a counted token then fails the call
(unless `only` filters the null away).

Per counted token (T, n): row[T].kmers += n (the row comes into being even if n is 0); on the first counted token of its line
row[K].reads += 1 for the line's class K, and row[K].kmersInMatchingReads += n if T == K.  `only` filters rows by key.
Rows come back in the order of DigitTrie.collect: byte-lexicographic, a prefix before its extensions.

A line of more than LONG_LINE bytes with its newline makes the reference fail (array index): long_lines="fail" states that,
long_lines="count" (what the project does) counts the line like any other and reports it in totals["long_lines"]."""
import re

LONG_LINE = 65536


class FormatError(Exception):
    """where the reference throws: .line is the 1-based line of the stream"""

    def __init__(self, line, what):
        super().__init__(f"line {line}: {what}")
        self.line = line
        self.what = what


_NUM = rb"(?:0|[1-9][0-9]{0,8})"
_TOK = rb"(?:A|" + _NUM + rb"):" + _NUM
# the lines the device counts itself (gs_krakencount.hip): everything else goes to the host's reference-exact parser
GRAMMAR = re.compile(rb"[^\t \x00\r\n\x80-\xff]*\t[^\t \x00\r\n]*\t(" + _NUM + rb")\t" + _NUM + rb"\t((?:" + _TOK + rb"(?: " + _TOK + rb")*)?)")


def in_grammar(line):
    """line: bytes without the newline"""
    return GRAMMAR.fullmatch(line) is not None


def _int(b, line):
    """ByteArrayUtil.byteArrayToInt: a Java int, wrapping"""
    v = 0
    for c in b:
        d = c - 48
        if d < 0 or d > 9:
            raise FormatError(line, f"non-digit in number {bytes(b)!r}")
        v = (v * 10 + d) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def _digits(b):
    return all(48 <= c <= 57 for c in b)


def lines(data, long_lines="count"):
    """the lines the reference's loop sees: (1-based number, bytes without the dropped last byte, bytes in the stream), up to where
    it ends"""
    data = bytes(data)
    pos, no = 0, 0
    while pos < len(data):
        j = data.find(b"\n", pos)
        raw = data[pos:] if j < 0 else data[pos:j + 1]
        pos += len(raw)
        kept = raw.replace(b"\0", b"")
        no += 1
        if len(kept) > LONG_LINE and long_lines == "fail":
            raise FormatError(no, "line longer than the reference's buffer")
        if len(kept) - 1 <= 0:
            return
        yield no, kept[:-1], len(kept)


def _line_tokens(no, ch, cls):
    """the state machine over one line -> (class key behind it, [(tax id key, count, class key at the time)] of the listener's
    calls, skipped 'A' tokens).  cls: the class key in front of the line"""
    start, descriptor, class_id, read_size, fr = True, False, False, False, False
    start_pos = fr_start = 0
    calls, n_a = [], 0
    n = len(ch)

    def close(end):
        nonlocal n_a, cls
        fr_n = _int(ch[fr_start:end], no)
        if ch[start_pos:start_pos + 1] == b"A":
            n_a += 1
            return
        # (the count has parsed, so its ':' lies behind start_pos: a count that began in front of it would hold the delimiter)
        key = ch[start_pos:fr_start - 1]
        if _digits(key):
            calls.append((key, fr_n, cls))

    for i in range(n):
        c = ch[i]
        if c == 9:
            if start:
                start, descriptor = False, True
            elif descriptor:
                descriptor, class_id = False, True
                start_pos = i + 1
            elif class_id:
                class_id, read_size = False, True
                cls = ch[start_pos:i]
                if not _digits(cls):
                    raise FormatError(no, f"non-digit in the class {cls!r}")
                start_pos = i + 1
            elif read_size:
                read_size = False
                _int(ch[start_pos:i], no)
                start_pos = i + 1
        elif c == 58:
            fr, fr_start = True, i + 1
        elif fr and c == 32:
            close(i)
            start_pos = i + 1
    if start_pos < n and fr:
        close(n)
    return cls, calls, n_a


def count(data, only=None, long_lines="count", fast=True):
    """(rows, totals) of one stream.  rows: [(key bytes, reads, kmers, kmers in matching reads)] in the reference's order; totals:
    lines, counted tokens, skipped 'A' tokens, long lines.  only: an iterable of keys (bytes or str) or None.  fast: lines inside
    GRAMMAR are split instead of walked (tests/test_krakencount_cpu.py holds the two against each other)."""
    allowed = None if only is None else {k.encode() if isinstance(k, str) else bytes(k) for k in only}
    rows = {}
    totals = {"lines": 0, "counted": 0, "a_tokens": 0, "long_lines": 0}

    def row(key):
        return rows.setdefault(key, [0, 0, 0])

    last_cls = None  # the reference's classTaxid lives across lines: a token in front of the third tab sees the class of the line before
    for no, ch, size in lines(data, long_lines):
        totals["lines"] += 1
        totals["long_lines"] += size > LONG_LINE
        m = GRAMMAR.fullmatch(ch) if fast else None
        if m is not None:
            last_cls, calls, n_a = m.group(1), [], 0
            for tok in m.group(2).split(b" ") if m.group(2) else ():
                key, _, cnt = tok.partition(b":")
                if key == b"A":
                    n_a += 1
                else:
                    calls.append((key, int(cnt), last_cls))
        else:
            last_cls, calls, n_a = _line_tokens(no, ch, last_cls)
        totals["a_tokens"] += n_a
        totals["counted"] += len(calls)
        for j, (key, cnt, cls) in enumerate(calls):
            if allowed is None or key in allowed:
                row(key)[1] += cnt
            if j == 0 and cls is None and allowed is None:
                raise FormatError(no, "a token on a line without a class")  # countingTrie.get(null, true) is null
            if j == 0 and (allowed is None or cls in allowed):
                r = row(cls)
                r[0] += 1
                if key == cls:
                    r[2] += cnt
    return [(k, *rows[k]) for k in sorted(rows)], totals


def csv(rows):
    """the krakenres file of KrakenResFileGoal: header, then key;reads;kmers;kmers in matching reads;"""
    out = [b"taxid;reads;kmers;kmers in matching reads\n"]
    out += [b"%s;%d;%d;%d;\n" % (k, r, km, ki) for k, r, km, ki in rows]
    return b"".join(out)
