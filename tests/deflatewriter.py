"""A DEFLATE writer for tests (RFC 1951): blocks are written from explicit code lengths and explicit tokens, so that a test can state
streams no compressor on this machine writes -- a lone distance code, no distance code, deep skewed codes, length 258 as symbol 284 + 31,
empty blocks, odd headers -- and streams that are damaged in exactly one way.  Plain Python; zlib is only used for CRC-32.

A token is a literal byte (int) or a match (length, distance) / (length, distance, True) -- the third field sends a length of 258 as
symbol 284 with extra bits 31.  Three more token forms exist for damaged streams: ("raw", value, nbits), ("lsym", symbol) and
("dsym", symbol) write bits / one literal-length code / one distance code and nothing else.

The writer records (bit position, bits, bytes of text) of every literal and match it wrote (Deflate.records) and the bit position of every
block header (Deflate.blocks), so a case can assert what it covers."""
import struct
import zlib

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def length_symbol(length, alt=False):
    """-> (symbol - 257, extra value) of a match length 3 .. 258"""
    assert 3 <= length <= 258
    if length == 258:
        return (27, 31) if alt else (28, 0)
    s = 28
    while LEN_BASE[s] > length:
        s -= 1
    if s == 28:
        s = 27
    return s, length - LEN_BASE[s]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    s = 29
    while DIST_BASE[s] > dist:
        s -= 1
    return s, dist - DIST_BASE[s]


def canonical(lens):
    """codes of RFC 1951 3.2.2 from code lengths, already bit-reversed (ready to be written low bit first); no check of the lengths"""
    count = [0] * 17
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for ln in lens:
        if ln == 0:
            out.append(0)
            continue
        c = nxt[ln] & ((1 << ln) - 1)  # (an over-subscribed set overflows: the stream is damaged on purpose)
        nxt[ln] += 1
        out.append(int(format(c, "0%db" % ln)[::-1], 2))
    return out


def kraft(lens):
    """sum of 2^-len in units of 2^-15 (a complete code: 32768)"""
    return sum(1 << (15 - ln) for ln in lens if ln)


def chain_code(symbols):
    """{symbol: length}: lengths 1, 2, ..., n - 2, n - 1, n - 1 in the order given (16 symbols: 1 .. 14, 15, 15)"""
    n = len(symbols)
    assert 2 <= n <= 16
    return {s: (i + 1 if i < n - 1 else n - 1) for i, s in enumerate(symbols)}


def random_complete_code(rng, symbols, maxlen=15, skew=0.5):
    """{symbol: length} of a complete code (Kraft sum exactly 1): leaves are split until every symbol has one; with probability `skew`
    the deepest leaf that can still be split is taken (deep, lopsided codes), else a random one.  rng: random.Random"""
    n = len(symbols)
    assert 2 <= n <= (1 << maxlen)
    leaves = [0]
    while len(leaves) < n:
        can = [i for i, d in enumerate(leaves) if d < maxlen]
        if rng.random() < skew:
            deepest = max(leaves[i] for i in can)
            i = rng.choice([i for i in can if leaves[i] == deepest])
        else:
            i = rng.choice(can)
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    rng.shuffle(leaves)
    assert kraft(leaves) == 32768
    return dict(zip(symbols, leaves))


def lens_list(code, n):
    """a {symbol: length} code as the list of n lengths a block takes"""
    out = [0] * n
    for s, ln in code.items():
        out[s] = ln
    return out


def balanced_lens(used, n):
    """a complete code over the symbols `used` (of 0 .. n - 1) with lengths that differ by at most one"""
    used = sorted(used)
    if len(used) == 1:
        used = sorted(set(used) | {0 if used[0] else 1})
    k = len(used).bit_length() - 1
    short = (1 << (k + 1)) - len(used)
    out = [0] * n
    for i, s in enumerate(used):
        out[s] = k if i < short else k + 1
    return out


def apply(tokens, prior=b""):
    """the text a token list stands for (behind `prior`, which matches may reach into)"""
    out = bytearray(prior)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, d = t[0], t[1]
            assert 1 <= d <= len(out), (d, len(out))
            if d >= ln:
                out += out[len(out) - d:len(out) - d + ln]
            else:
                for _ in range(ln):
                    out.append(out[-d])
    return bytes(out[len(prior):])


def cl_plain(lens):
    """the lengths as code length symbols, one each"""
    return [(ln, 0) for ln in lens]


def cl_runs(lens):
    """the lengths as code length symbols with greedy 16 / 17 / 18 runs (over the whole sequence: a run crosses from the literal /
    length lengths into the distance lengths as it comes)"""
    out, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        j = i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
        i = j
    return out


class Deflate:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.nacc = 0
        self.records = []  # (bit position, bits, bytes of text) of every literal and match
        self.blocks = []   # (bit position of the header, "stored" / "fixed" / "dynamic")

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.nacc

    def bits(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.nacc
        self.nacc += n
        if self.nacc >= 64:
            k = self.nacc // 8
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.nacc -= 8 * k

    def align(self):
        self.bits(0, -self.bitpos % 8)

    def payload(self):
        return bytes(self.buf) + self.acc.to_bytes((self.nacc + 7) // 8, "little")

    # ---- blocks
    def stored(self, final, data, nlen=None):
        """(the 0 .. 7 bits of padding in front of LEN are whatever the bit position in front of the block makes them)"""
        assert len(data) <= 65535
        self.blocks.append((self.bitpos, "stored"))
        self.bits(int(bool(final)), 1)
        self.bits(0, 2)
        self.align()
        self.bits(len(data), 16)
        self.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        assert self.nacc % 8 == 0
        self.buf += self.acc.to_bytes(self.nacc // 8, "little")
        self.acc = self.nacc = 0
        self.buf += data
        return self

    def _tokens(self, tokens, lit_lens, dist_lens, alt258, eob):
        lc, dc = canonical(lit_lens), canonical(dist_lens)
        for t in tokens:
            at = self.bitpos
            if isinstance(t, int):
                assert lit_lens[t], "literal %d has no code" % t
                self.bits(lc[t], lit_lens[t])
                self.records.append((at, lit_lens[t], 1))
            elif t[0] == "raw":
                self.bits(t[1], t[2])
            elif t[0] == "lsym":
                self.bits(lc[t[1]], lit_lens[t[1]])
            elif t[0] == "dsym":
                self.bits(dc[t[1]], dist_lens[t[1]])
            else:
                ls, lx = length_symbol(t[0], alt258 or (len(t) > 2 and t[2]))
                ds, dx = dist_symbol(t[1])
                assert lit_lens[257 + ls] and dist_lens[ds], "match %r has no code" % (t,)
                self.bits(lc[257 + ls], lit_lens[257 + ls])
                self.bits(lx, LEN_EXTRA[ls])
                self.bits(dc[ds], dist_lens[ds])
                self.bits(dx, DIST_EXTRA[ds])
                self.records.append((at, self.bitpos - at, t[0]))
        if eob:
            self.bits(lc[256], lit_lens[256])

    def fixed(self, final, tokens, alt258=False, eob=True):
        self.blocks.append((self.bitpos, "fixed"))
        self.bits(int(bool(final)), 1)
        self.bits(1, 2)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST, alt258, eob)
        return self

    def dynamic(self, final, lit_lens, dist_lens, tokens, cl_lens=None, hclen=None, runs=False, alt258=False, cl_seq=None, eob=True):
        """lit_lens: 257 .. 286 lengths (HLIT = their number), dist_lens: 1 .. 30 (HDIST).  cl_lens: the 19 lengths of the code length
        code (default: a balanced code over the symbols the header uses); hclen: how many of them are sent (default: as few as the
        code allows, at least 4); runs: lengths as 16 / 17 / 18 runs; cl_seq: the (symbol, extra value) sequence itself"""
        self.blocks.append((self.bitpos, "dynamic"))
        seq = cl_seq if cl_seq is not None else (cl_runs if runs else cl_plain)(list(lit_lens) + list(dist_lens))
        if cl_lens is None:
            cl_lens = balanced_lens({s for s, _ in seq}, 19)
        assert len(cl_lens) == 19 and all(cl_lens[s] for s, _ in seq)
        need = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        hclen = need if hclen is None else hclen
        assert need <= hclen <= 19
        self.bits(int(bool(final)), 1)
        self.bits(2, 2)
        self.bits(len(lit_lens) - 257, 5)
        self.bits(len(dist_lens) - 1, 5)
        self.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.bits(cl_lens[s], 3)
        cc = canonical(cl_lens)
        for s, x in seq:
            self.bits(cc[s], cl_lens[s])
            if s >= 16:
                self.bits(x, (2, 3, 7)[s - 16])
        self._tokens(tokens, list(lit_lens) + [0] * (288 - len(lit_lens)), list(dist_lens) + [0] * (32 - len(dist_lens)), alt258, eob)
        return self


def gzip_member(payload, text):
    return b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + payload + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


def bgzf_member(payload, text):
    """one BGZF member (SAM spec 4.1) around a deflate payload"""
    assert len(payload) < 65536 - 26 and len(text) <= 65536, (len(payload), len(text))
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload +
            struct.pack("<II", zlib.crc32(text), len(text)))
