"""Hand-written inputs of the krakencount tests, with the rows worked out by hand from KrakenResultProcessor.java:74-179 and
KrakenResCountGoal.java:133-157.  A helper module of the suite, not a test file.

A case: name, data (one stream), only (None or keys), expect = rows [(key, reads, kmers, kmers in matching reads)] in the
reference's order or ("error", 1-based line), totals (lines, counted tokens, skipped 'A' tokens) or None, and for the device:
None if every line is inside its grammar, else the 0-based line that refuses the chunk."""
import collections

Case = collections.namedtuple("Case", "name data only expect totals bad_line")

LONG_LINE = 65536


def line(tokens, cls=b"9", desc=b"d", flag=b"C", size=b"100"):
    return flag + b"\t" + desc + b"\t" + cls + b"\t" + size + b"\t" + tokens + b"\n"


def long_line(n_bytes):
    """one line of n_bytes with its newline: class 9, token 9:5"""
    body = line(b"9:5", desc=b"")
    return line(b"9:5", desc=b"x" * (n_bytes - len(body)))


GOLDEN = b"C\ttest\t1\t41\t0:2 1:7 0:2\n"  # tests/golden/dengue1/test.out

CASES = [
    # class 1; the first counted token is 0:2, not of the class: reads[1] = 1, nothing matches
    Case("golden", GOLDEN, None, [(b"0", 0, 4, 0), (b"1", 1, 7, 0)], (1, 3, 0), None),
    # the descriptor's ':' arms fr early; the first token's own ':' sets the count's start
    Case("descriptor_colon", line(b"9:5 3:2", desc=b"A01245:102:x"), None, [(b"3", 0, 2, 0), (b"9", 1, 5, 5)], (1, 2, 0), None),
    Case("a_first", line(b"A:4 9:5 3:2"), None, [(b"3", 0, 2, 0), (b"9", 1, 5, 5)], (1, 2, 1), None),
    Case("a_middle", line(b"9:5 A:4 3:2"), None, [(b"3", 0, 2, 0), (b"9", 1, 5, 5)], (1, 2, 1), None),
    Case("a_last", line(b"9:5 3:2 A:4"), None, [(b"3", 0, 2, 0), (b"9", 1, 5, 5)], (1, 2, 1), None),
    # a count of 0 still makes the row
    Case("zero_count", line(b"5:0"), None, [(b"5", 0, 0, 0), (b"9", 1, 0, 0)], (1, 1, 0), None),
    Case("class_is_first_token", line(b"9:5 9:2"), None, [(b"9", 1, 7, 5)], (1, 2, 0), None),
    # only the FIRST counted token can match the class
    Case("class_is_later_token", line(b"9:5 3:2", cls=b"3"), None, [(b"3", 1, 2, 0), (b"9", 0, 5, 0)], (1, 2, 0), None),
    Case("only_a_tokens", line(b"A:7 A:3", cls=b"0", flag=b"U"), None, [], (1, 0, 2), None),
    Case("no_tokens", line(b"") + line(b"9:1"), None, [(b"9", 1, 1, 1)], (2, 1, 0), None),
    # keys are strings
    Case("leading_zeros", line(b"7:5 007:2", cls=b"007"), None, [(b"007", 1, 2, 0), (b"7", 0, 5, 0)], (1, 2, 0), 0),
    Case("empty_class", line(b"7:5", cls=b""), None, [(b"", 1, 0, 0), (b"7", 0, 5, 0)], (1, 1, 0), 0),
    # the caught IllegalStateException: the token is skipped, the next one is the line's first counted one
    Case("nondigit_taxid", line(b"9x:5 9:2"), None, [(b"9", 1, 2, 2)], (1, 1, 0), 0),
    Case("nondigit_count", line(b"9:5") + line(b"9:5x 3:1"), None, ("error", 2), None, 1),
    Case("nondigit_size", line(b"9:5", size=b"1x0"), None, ("error", 1), None, 0),
    Case("nondigit_class", line(b"9:5") + line(b"9:5") + line(b"9:5", cls=b"9a"), None, ("error", 3), None, 2),
    Case("crlf", line(b"9:5")[:-1] + b"\r\n", None, ("error", 1), None, 0),
    # the second blank closes a token whose count would be "5 "
    Case("double_blank", line(b"9:5  3:1"), None, ("error", 1), None, 0),
    # a blank at the end closes the last token, and nothing is left to close at the end of the line
    Case("trailing_blank", line(b"9:5 "), None, [(b"9", 1, 5, 5)], (1, 1, 0), 0),
    # a blank in the descriptor behind a ':' closes a "token" there: 22:7 counts, and is the line's first counted token -- in
    # front of the line's own class field, so under the class of the line before (5); on a first line that class is null
    Case("descriptor_token", line(b"9:5", cls=b"5") + line(b"0:1", cls=b"7", desc=b"d1:5 22:7 z"), None,
         [(b"0", 0, 1, 0), (b"22", 0, 7, 0), (b"5", 2, 0, 0), (b"9", 0, 5, 0)], (2, 3, 0), 1),
    Case("descriptor_token_first_line", line(b"0:1", cls=b"7", desc=b"d1:5 22:7 z"), None, ("error", 1), None, 0),
    Case("descriptor_token_filtered", line(b"0:1", cls=b"7", desc=b"d1:5 22:7 z"), [b"22", b"7"], [(b"22", 0, 7, 0)], (1, 2, 0), 0),
    # a fifth tab is no delimiter: the one token of the line is "9:5\t3:1", tax id "9:5\t3", skipped
    Case("five_tabs", line(b"9:5\t3:1"), None, [], (1, 0, 0), 0),
    # without a fourth tab the size field holds the token
    Case("three_tabs", b"C\td\t9\t9:5\n", None, [(b"9", 1, 5, 5)], (1, 1, 0), 0),
    Case("ten_digits", line(b"1234567890:1"), None, [(b"1234567890", 0, 1, 0), (b"9", 1, 0, 0)], (1, 1, 0), 0),
    # the loop ends at the first empty line
    Case("empty_line", line(b"9:5") + b"\n" + line(b"9:7"), None, [(b"9", 1, 5, 5)], (1, 1, 0), None),
    Case("empty_line_first", b"\n" + line(b"9:7"), None, [], (0, 0, 0), None),
    # an unterminated last line loses its last byte: 9:73 counts as 9:7
    Case("no_final_newline", line(b"9:5") + line(b"9:73")[:-1], None, [(b"9", 2, 12, 12)], (2, 2, 0), 1),
    Case("one_byte_tail", line(b"9:5") + b"x", None, [(b"9", 1, 5, 5)], (1, 1, 0), 1),
    # NUL bytes are dropped
    Case("nul", line(b"9:\x005"), None, [(b"9", 1, 5, 5)], (1, 1, 0), 0),
    # `only` selects rows by key: token rows and class rows alike
    Case("only_segment_key", line(b"9:5 3:2"), [b"3"], [(b"3", 0, 2, 0)], (1, 2, 0), None),
    Case("only_class_key", line(b"9:5 3:2"), [b"9"], [(b"9", 1, 5, 5)], (1, 2, 0), None),
    Case("row_order", line(b"2:1 11:1 10:1 1:1", cls=b"1"), None, [(b"1", 1, 1, 0), (b"10", 0, 1, 0), (b"11", 0, 1, 0), (b"2", 0, 1, 0)], (1, 4, 0), None),
    # sums beyond 2^32
    Case("big_sums", line(b"7:999999999", cls=b"7") * 5, None, [(b"7", 5, 4999999995, 4999999995)], (5, 5, 0), None),
    # the longest line the reference takes
    Case("line_65536", long_line(LONG_LINE), None, [(b"9", 1, 5, 5)], (1, 1, 0), None),
]


def random_line(rng, taxids, pad=0):
    """one line inside the device's grammar; pad: extra descriptor bytes"""
    n_tok = int(rng.integers(0, 6))
    toks = []
    for _ in range(n_tok):
        u = rng.random()
        key = b"A" if u < 0.15 else b"0" if u < 0.55 else str(int(rng.choice(taxids))).encode()
        toks.append(key + b":" + str(int(rng.integers(0, 200))).encode())
    cls = b"0" if rng.random() < 0.3 else str(int(rng.choice(taxids))).encode()
    desc = b"r" + str(int(rng.integers(0, 10 ** 6))).encode() + (b":1:2" if rng.random() < 0.3 else b"") + b"x" * pad
    return line(b" ".join(toks), cls=cls, desc=desc, flag=b"C" if cls != b"0" else b"U", size=str(int(rng.integers(1, 300))).encode())


def random_text(rng, n_bytes, taxids=(1, 7, 10, 11, 562, 1280, 9606, 999999999)):
    """exactly n_bytes (>= 64) of lines inside the device's grammar"""
    out, size = [], 0
    pool = [random_line(rng, taxids) for _ in range(min(2000, n_bytes // 40 + 1))]  # (a large text repeats lines of a pool)
    for i in rng.integers(0, len(pool), size=n_bytes // 12):
        if n_bytes - size < 128:
            break
        out.append(pool[i])
        size += len(out[-1])
    last = random_line(rng, taxids)
    while len(last) > n_bytes - size:
        last = line(b"")
    out.append(last[:2] + b"x" * (n_bytes - size - len(last)) + last[2:])
    text = b"".join(out)
    assert len(text) == n_bytes
    return text


def first_empty_line(data):
    """byte offset of the first empty line of a text, -1 if it has none"""
    return 0 if data.startswith(b"\n") else data.find(b"\n\n") + 1 if b"\n\n" in data else -1


def sample_reads(genomes, n, rng):
    """n reads of mixed lengths for the identity tests: pieces of the genomes (uint8 [species, length]), some with a mutation or a
    run of N, a fifth random, some shorter than k = 31 -> [(descriptor line, read)]"""
    out = []
    for i in range(n):
        L = int(rng.choice((20, 31, 75, 150, 151, 300)))
        if i % 5 == 0:
            r = bytes(b"ACGT"[x] for x in rng.integers(0, 4, L))
        else:
            g = genomes[int(rng.integers(0, genomes.shape[0]))]
            p = int(rng.integers(0, g.shape[0] - L))
            r = bytearray(g[p:p + L].tobytes())
            if i % 7 == 0 and L > 40:
                q = int(rng.integers(0, L - 8))
                r[q:q + int(rng.integers(1, 8))] = b"N" * len(r[q:q + int(rng.integers(1, 8))])
            if i % 11 == 0:
                r[L // 2] = ord("ACGT"[(b"ACGT".index(r[L // 2]) + 1) % 4]) if r[L // 2] in b"ACGT" else r[L // 2]
            r = bytes(r)
        out.append((b"@r%d:%d x=%d" % (i, L, i % 3), r))
    return out


def check_identities(rows, table, taxids):
    """what a Kraken-style file of a match run must add up to (FastqKMerMatcher.java:390-413, 452-473: every hit contig goes once
    to stats.kmers and once to the line's segments; a classified read's line carries its class): for every tax id T of the store,
    kmers of T == the table's "kmers" column, reads of T == its "reads" column (maxReadClassErrorCount < 0)"""
    by_key = {k: (r, km) for k, r, km, _ in rows}
    assert len(set(taxids)) == len(taxids) and "0" not in taxids
    for vi, t in enumerate(taxids):
        reads, kmers = by_key.get(t.encode(), (0, 0))
        assert kmers == int(table[vi, 2]), (t, kmers, int(table[vi, 2]))
        assert reads == int(table[vi, 0]), (t, reads, int(table[vi, 0]))
    assert set(by_key) <= {t.encode() for t in taxids} | {b"0"}
