"""The catalogue of DEFLATE streams that zlib never writes (tests/deflatewriter.py writes them; zlib.decompress is the reference for every
one): the smallest shapes at which each mechanism of the decoders -- gs_inflate_members / gs_gunzip_device on the device, GsGunzip /
GsParallelGunzip on the host -- can go wrong.  legal() and rejected() return lists of Case, built once from fixed seeds.

A Case has a name, a group, the deflate payload and the text.  Unless `gzip_only`, the payload fits one BGZF member.  `any_bytes`: bytes
>= 128 have codes (the block finder of the single-member path takes such block starts only with GS_GUNZIP_ANY_BYTES=1).  `cover` holds
what the case asserts about itself (tests/test_inflate_cases_cpu.py checks the conditions)."""
import functools
import gzip
import random

import deflatewriter as dw

A, C, G, T, NL, N = 65, 67, 71, 84, 10, 78


class Case:
    def __init__(self, name, group, payload, text, any_bytes=False, gzip_only=False, cover=None):
        self.name, self.group, self.payload, self.text = name, group, payload, text
        self.any_bytes, self.gzip_only, self.cover = any_bytes, gzip_only, cover or {}
        if not gzip_only:
            dw.bgzf_member(payload, text)  # (asserts the sizes)

    def __repr__(self):
        return "Case(%s)" % self.name


def _lens(pairs, n):
    return dw.lens_list(dict(pairs), n)


def _hlit(lens):
    """the literal / length lengths cut to HLIT: behind the last code, at least 257"""
    n = max(257, max(i for i, v in enumerate(lens) if v) + 1)
    return lens[:n]


def _hdist(lens):
    n = max([1] + [i + 1 for i, v in enumerate(lens) if v])
    return lens[:n]


def _used_code(tokens, extra_lit=(), alt258=False):
    """balanced codes over exactly what the tokens use (plus the end-of-block code): -> (lit_lens cut to HLIT, dist_lens cut to HDIST);
    no match: no distance code at all; one distance symbol: the lone 1-bit code"""
    lits, dists = {256} | set(extra_lit), set()
    for t in tokens:
        if isinstance(t, int):
            lits.add(t)
        else:
            lits.add(257 + dw.length_symbol(t[0], alt258 or (len(t) > 2 and t[2]))[0])
            dists.add(dw.dist_symbol(t[1])[0])
    ll = dw.balanced_lens(lits, 288)
    if len(dists) == 0:
        dl = [0]
    elif len(dists) == 1:
        dl = _hdist(dw.lens_list({next(iter(dists)): 1}, 32))
    else:
        dl = _hdist(dw.balanced_lens(dists, 32))
    return _hlit(ll), dl


def _acgt(rng, n):
    return [rng.choice((A, C, G, T)) for _ in range(n)]


# ---- one_dist_code / no_dist_code
def _one_dist_code():
    out = []
    for name, sym in (("sym0", 0), ("sym10", 10), ("sym29", 29)):
        rng = random.Random(100 + sym)
        d = dw.Deflate()
        prior = b""
        if sym == 29:  # distances of 24577 and more need that much text in front: a stored block (the matches reach into it)
            prior = bytes(rng.choice(b"ACGTN\n") for _ in range(25000))
            d.stored(False, prior)
        tokens = _acgt(rng, 60)
        pos = len(prior) + 60
        lo, hi = dw.DIST_BASE[sym], dw.DIST_BASE[sym] + (1 << dw.DIST_EXTRA[sym]) - 1
        for k in range(500):
            ln = rng.randint(3, 258) if k % 5 == 0 else rng.randint(3, 20)
            if pos + ln + 4 > 65000:
                break
            tokens.append((ln, rng.randint(lo, min(hi, pos))))
            fresh = _acgt(rng, rng.randint(0, 3))
            tokens += fresh
            pos += ln + len(fresh)
        ll = _hlit(dw.balanced_lens({A, C, G, T, 256} | set(range(257, 286)), 288))
        dl = _hdist(dw.lens_list({sym: 1}, 32))
        d.dynamic(True, ll, dl, tokens)
        out.append(Case("one_dist_code_" + name, "one_dist_code", d.payload(), prior + dw.apply(tokens, prior)))
    return out


def _no_dist_code():
    rng = random.Random(7)
    tokens = list(range(256)) + [rng.randrange(256) for _ in range(5000)]
    ll = dw.balanced_lens(set(range(257)), 288)[:257]
    d = dw.Deflate().dynamic(True, ll, [0], tokens)
    return [Case("no_dist_code", "no_dist_code", d.payload(), dw.apply(tokens), any_bytes=True)]


# ---- deep48: a literal / length symbol of 15 bits with 5 extra bits next to a distance symbol of 15 bits with 13 extra bits
def _deep48():
    out = []
    lit_code = dw.chain_code([A, C, G, T, NL, N, 64, 43, 70, 58, 44, 35, 256, 257, 281, 282])  # 281, 282 (131 .. 194 bytes): 15 bits
    dist_code = dw.chain_code([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 28, 29])            # 28, 29 (16385 .. 32768): 15 bits
    ll, dl = _hlit(dw.lens_list(lit_code, 288)), _hdist(dw.lens_list(dist_code, 32))
    for seed in range(4):
        rng = random.Random(480 + seed)
        lits = [A, C, G, T, NL, N, 64, 43, 70]
        tokens = [rng.choice(lits[:4 + seed]) for _ in range(16400 + 13 * seed)]
        pos = len(tokens)
        while pos + 200 < 65536:
            ln = rng.randint(131, 194)
            tokens.append((ln, rng.randint(16385, min(32768, pos))))
            pos += ln
            for _ in range(rng.choice((0, 0, 1, 1, 2, 3))):
                tokens.append(rng.choice(lits))
                pos += 1
        d = dw.Deflate().dynamic(True, ll, dl, tokens)
        deep = [(at, n) for at, n, _ in d.records if n == 48]
        cover = dict(deep=len(deep), offsets=sorted({at % 32 for at, _ in deep}),
                     straddle=sum(1 for at, n in deep if at // 2048 != (at + n - 1) // 2048))
        out.append(Case("deep48_%d" % seed, "deep48", d.payload(), dw.apply(tokens), cover=cover))
    return out


# ---- random_codes: fresh random complete codes over all of 0 .. 285 and 0 .. 29
def random_member(rng, name, group="random_codes", max_text=65536, max_payload=60000):
    d = dw.Deflate()
    text = bytearray()
    blocks = []
    full = False
    while not full:
        skew = rng.choice((0.0, 0.5, 0.9, 0.98))
        ll = dw.lens_list(dw.random_complete_code(rng, list(range(286)), 15, skew), 286)
        dl = dw.lens_list(dw.random_complete_code(rng, list(range(30)), 15, rng.choice((0.0, 0.5, 0.9, 0.98))), 30)
        tokens = []
        for _ in range(rng.randint(200, 3000)):
            if text and rng.random() < 0.35:
                ln = rng.randint(3, 10) if rng.random() < 0.7 else rng.randint(3, 258)
                dist = rng.randint(1, min(len(text), 32768))
                t = (ln, dist)
                if len(text) + ln > max_text:
                    full = True
                    break
                for _ in range(ln):
                    text.append(text[-dist])
            else:
                t = rng.randrange(256)
                if len(text) + 1 > max_text:
                    full = True
                    break
                text.append(t)
            tokens.append(t)
        # (a token takes at most 48 bits, a header less than 400 bytes: the payload stays under a BGZF member's limit; the text of a
        # block that is not written is cut off again below)
        if d.bitpos // 8 + 6 * len(tokens) + 400 > max_payload:
            break
        blocks.append(tokens)
        d.dynamic(False, ll, dl, tokens, runs=rng.random() < 0.5)
    d.fixed(True, [])
    n = sum(1 if isinstance(t, int) else t[0] for b in blocks for t in b)
    return Case(name, group, d.payload(), bytes(text[:n]), any_bytes=True, cover=dict(blocks=len(blocks)))


def _random_codes():
    return [random_member(random.Random(9000 + i), "random_codes_%02d" % i) for i in range(40)]


# ---- dense: literal code mass against the threshold of the four-tokens-at-a-time walk (half the code space in literals of <= 3 bits)
_DENSE_CODES = {
    "one_1bit": [(A, 1)] + [(s, 4) for s in (C, G, T, NL, 256, 257, 258, 259)],                  # mass 4/8: at the threshold
    "two_2bit": [(A, 2), (C, 2)] + [(s, 4) for s in (G, T, NL, N, 256, 257, 258, 259)],          # at the threshold
    "four_3bit": [(s, 3) for s in (A, C, G, T)] + [(s, 4) for s in (NL, N, 64, 256, 257, 258, 259, 260)],  # at the threshold
    "three_3bit": [(s, 3) for s in (A, C, G)] + [(s, 4) for s in (T, NL, N, 64, 43, 256, 257, 258, 259, 260)],  # 3/8: just below
    "well_above": [(A, 1), (C, 2), (G, 3), (T, 4), (256, 5), (257, 5)],                          # 7/8
}


def dense_mass(lit_lens):
    """literal code mass in eighths of the code space, as the decoder sums it"""
    return sum(8 >> v for v in lit_lens[:256] if 1 <= v <= 3)


def _dense():
    out = []
    dl = [3] * 8  # distances 1 .. 16
    for name, pairs in _DENSE_CODES.items():
        rng = random.Random(sum(map(ord, name)))
        ll = _hlit(_lens(pairs, 288))
        lits = [s for s, _ in pairs if s < 256]
        wts = [2.0 ** -v for s, v in pairs if s < 256]
        lens_ok = [3 + s - 257 for s, _ in pairs if s >= 257]
        tokens = rng.choices(lits, wts, k=20)
        for _ in range(6000):
            if rng.random() < 0.12:
                tokens.append((rng.choice(lens_ok), rng.randint(1, 16)))
            else:
                tokens.append(rng.choices(lits, wts)[0])
        d = dw.Deflate()
        third = len(tokens) // 3
        d.dynamic(False, ll, dl, tokens[:third]).dynamic(False, ll, dl, tokens[third:2 * third], runs=True).dynamic(True, ll, dl, tokens[2 * third:])
        out.append(Case("dense_" + name, "dense", d.payload(), dw.apply(tokens), cover=dict(mass=dense_mass(ll))))
    # the 1-bit literal: blocks of 1 .. 130 literals, so that the end-of-block code stands at every lane of a group
    ll = _hlit(_lens(_DENSE_CODES["one_1bit"], 288))
    d, tokens = dw.Deflate(), []
    for n in range(1, 131):
        blk = [A] * n
        if n % 7 == 0:
            blk[n // 2] = C
        d.dynamic(False, ll, dl, blk)
        tokens += blk
    d.dynamic(True, ll, dl, [G])
    tokens.append(G)
    out.append(Case("dense_eob_every_lane", "dense", d.payload(), dw.apply(tokens), cover=dict(mass=dense_mass(ll))))
    return out


# ---- first_group_sizes: the first 64 bits of a block hold one match and 1-bit literals: groups of 250 .. 262 symbols (GI_LANE_SYMS = 256),
# and groups of more than 256 with a second match of 15 .. 18 bytes in front (GI_PAR_MAX = 16)
def _first_group_sizes():
    out = []
    ll = _hlit(_lens([(A, 1), (283, 3), (256, 3), (C, 3), (G, 3)], 288))  # 283: lengths 195 .. 226, five extra bits
    for variant, dl in (("run", [1]), ("far", _hdist(dw.lens_list({0: 1, 8: 1}, 32)))):
        rng = random.Random(250 if variant == "run" else 251)
        d = dw.Deflate()
        tokens = [rng.choice((A, C, G)) for _ in range(48)]
        d.dynamic(False, ll, dl, tokens)
        totals = []
        for total in range(250, 263):
            # 'C' (3 bits), the match (3 + 5 + 1 bits, and 3 extra bits of the distance in the second variant), 'A' to the 64th bit
            mbits = 9 if variant == "run" else 12
            n_a = 64 - 3 - mbits
            dist = 1 if variant == "run" else rng.randint(17, 24)
            blk = [C, (total - 1 - n_a, dist)] + [A] * n_a + [G, C, A, A, G]
            d.dynamic(False, ll, dl, blk)
            tokens += blk
            totals.append(total)
        d.dynamic(True, ll, dl, [G])
        tokens.append(G)
        out.append(Case("first_group_sizes_" + variant, "first_group_sizes", d.payload(), dw.apply(tokens), cover=dict(totals=totals)))
    # more than 256 symbols in the group, and a match of 15 .. 18 bytes in front of the long one: short enough / too long to be copied
    # one lane per match
    ll = _hlit(_lens([(A, 1), (283, 3), (G, 3), (267, 4), (268, 4), (256, 4), (C, 4)], 288))  # 267: 15, 16; 268: 17, 18
    dl = _hdist(dw.lens_list({0: 1, 8: 1}, 32))
    rng = random.Random(252)
    d = dw.Deflate()
    tokens = [rng.choice((A, C, G)) for _ in range(48)]
    d.dynamic(False, ll, dl, tokens)
    shorts = []
    for total in (257, 280):
        for m in (15, 16, 17, 18):
            for short_first in (True, False):
                # 'C' (4), short match (4 + 1 + 1 + 3), long match at distance 1 (3 + 5 + 1), 'A' to the 64th bit
                n_a = 64 - 4 - 9 - 9
                short, long_ = (m, rng.randint(20, 24)), (total - 1 - m - n_a, 1)
                blk = [C] + ([short, long_] if short_first else [long_, short]) + [A] * n_a + [G, C, A, A, G]
                d.dynamic(False, ll, dl, blk)
                tokens += blk
                shorts.append((total, m, short_first))
    d.dynamic(True, ll, dl, [G])
    tokens.append(G)
    out.append(Case("first_group_sizes_short_matches", "first_group_sizes", d.payload(), dw.apply(tokens), cover=dict(shorts=shorts)))
    return out


# ---- alt258: length 258 as symbol 284 with extra bits 31
def _alt258():
    rng = random.Random(258)
    tokens = _acgt(rng, 1000)
    pos = 1000
    n_alt = n_plain = 0
    for k in range(150):
        alt = k % 3 != 2
        dist = (1, 2, 7, rng.randint(258, min(pos, 32768)), rng.randint(1, 257))[k % 5]
        tokens.append((258, dist, alt))
        n_alt += alt
        n_plain += not alt
        fresh = _acgt(rng, rng.randint(0, 3))
        tokens += fresh
        pos += 258 + len(fresh)
    half = len(tokens) // 2
    d = dw.Deflate().fixed(False, tokens[:half])
    ll, dl = _used_code(tokens[half:], extra_lit=(284, 285))
    d.dynamic(False, ll, dl, tokens[half:])
    every = [(258, 1)] * 20 + [A, (258, 300)] * 10  # ... and a block in which every 258 goes the long way
    ll2, dl2 = _used_code(every, alt258=True)
    d.dynamic(True, ll2, dl2, every, alt258=True)
    return [Case("alt258", "alt258", d.payload(), dw.apply(tokens + every), cover=dict(alt=n_alt + 30, plain=n_plain))]


# ---- tiny_blocks: hundreds of blocks of 0 .. 5 tokens of all three kinds
def _tiny_blocks():
    rng = random.Random(600)
    d = dw.Deflate()
    text = bytearray()
    kinds = {"stored": 0, "fixed": 0, "dynamic": 0}
    empty = {"stored": 0, "fixed": 0, "dynamic": 0}
    into_stored = across = 0
    last_stored = (0, 0)  # [from, to) of the text of the last stored block
    for i in range(600):
        kind = ("stored", "fixed", "dynamic")[i % 3] if i < 30 else rng.choice(("stored", "fixed", "dynamic"))
        n = 0 if i % 10 == 3 else rng.randint(0, 5)
        kinds[kind] += 1
        empty[kind] += n == 0
        if kind == "stored":
            data = bytes(rng.choice(b"ACGT\n") for _ in range(n))
            last_stored = (len(text), len(text) + n)
            d.stored(False, data)
            text += data
            continue
        tokens, start = [], len(text)
        for _ in range(n):
            if len(text) >= 4 and rng.random() < 0.5:
                ln = rng.randint(3, 10)
                if last_stored[1] > last_stored[0] and rng.random() < 0.3:
                    dist = len(text) - rng.randrange(last_stored[0], last_stored[1])
                    into_stored += 1
                else:
                    dist = rng.randint(1, min(len(text), 60))
                across += dist > len(text) - start
                tokens.append((ln, dist))
                for _ in range(ln):
                    text.append(text[-dist])
            else:
                tokens.append(rng.choice((A, C, G, T, NL)))
                text.append(tokens[-1])
        if kind == "fixed":
            d.fixed(False, tokens)
        else:
            ll, dl = _used_code(tokens)
            d.dynamic(False, ll, dl, tokens, runs=rng.random() < 0.5)
    d.fixed(True, [])  # the final block is empty
    pads = sorted({-(at + 3) % 8 for at, kind in d.blocks if kind == "stored"})
    return [Case("tiny_blocks", "tiny_blocks", d.payload(), bytes(text),
                 cover=dict(kinds=kinds, empty=empty, pads=pads, into_stored=into_stored, across=across, blocks=len(d.blocks)))]


# ---- stored_extremes (gzip only: more text than a BGZF member holds)
def _stored_extremes():
    rng = random.Random(65535)
    a = bytes(rng.choice(b"ACGTN\n@+F:") for _ in range(65535))
    b = bytes(rng.choice(b"ACGT") for _ in range(65535))
    prior = a + b + b"\n"
    d = dw.Deflate().stored(False, a).stored(False, b"").stored(False, b).stored(False, b"\n")
    tokens = []
    for k in range(300):
        tokens.append((rng.randint(3, 258), 32768 - (k % 3)))
        tokens += _acgt(rng, rng.randint(0, 2))
    ll, dl = _used_code(tokens)
    d.dynamic(True, ll, dl, tokens)
    return [Case("stored_extremes", "stored_extremes", d.payload(), prior + dw.apply(tokens, prior), gzip_only=True)]


# ---- header_extremes
def _header_extremes():
    out = []
    rng = random.Random(286)

    def add(name, d, tokens, **kw):
        out.append(Case("header_" + name, "header_extremes", d.payload(), dw.apply(tokens), **kw))

    # HLIT = 257 with HDIST = 1 (the lone code: distance 1)
    # (HLIT = 257: no length code, so no match; the distance code is sent all the same)
    tokens = _acgt(rng, 2000)
    ll = _lens([(A, 2), (C, 2), (G, 3), (T, 3), (256, 3), (250, 3)], 288)[:257]
    add("hlit257_hdist1", dw.Deflate().dynamic(True, ll, [1], tokens), tokens, any_bytes=True)
    # HLIT = 286 with HDIST = 30: every symbol has a code
    ll = dw.lens_list(dw.random_complete_code(rng, list(range(286)), 12, 0.3), 286)
    dl = dw.lens_list(dw.random_complete_code(rng, list(range(30)), 9, 0.3), 30)
    tokens = [rng.randrange(256) for _ in range(300)]
    for _ in range(1500):
        tokens.append((rng.randint(3, 258), rng.randint(1, 300)) if rng.random() < 0.2 else rng.randrange(256))
    add("hlit286_hdist30", dw.Deflate().dynamic(True, ll, dl, tokens, hclen=19), tokens, any_bytes=True)
    # a code length code with 7-bit codes: the lengths 0 .. 7 under the chain 1, 2, ..., 7, 7
    ll = _hlit(dw.lens_list(dw.chain_code([A, C, G, T, NL, 256, 257, 258]), 288))  # lengths 1 .. 7, 7
    dl = _hdist(dw.lens_list(dw.chain_code([0, 1, 2, 3]), 32))                      # 1, 2, 3, 3
    cl = dw.lens_list(dw.chain_code([0, 1, 2, 3, 4, 5, 6, 7]), 19)                  # symbol 0: one bit ... symbols 6, 7: seven bits
    tokens = _acgt(rng, 30) + [(rng.randint(3, 4), rng.randint(1, 4)) if i % 5 == 0 else rng.choice((A, C, G, T, NL)) for i in range(3000)]
    for name, hclen in (("cl7_minimal", None), ("cl7_hclen19", 19)):
        add(name, dw.Deflate().dynamic(True, ll, dl, tokens, cl_lens=cl, hclen=hclen), tokens)
    # a flat code length code: sixteen codes of four bits for the lengths 0 .. 15, no run symbols, all 19 lengths sent
    ll15 = _hlit(dw.lens_list(dw.chain_code([A, C, G, T, NL, N, 64, 43, 70, 58, 44, 35, 256, 257, 258, 259]), 288))  # lengths 1 .. 15, 15
    dl15 = _hdist(dw.lens_list(dw.chain_code([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]), 32))
    tokens = _acgt(rng, 300) + [(rng.randint(3, 5), rng.randint(1, 256)) if i % 3 == 0 else rng.choice((A, C, G, T, NL, N, 64, 43, 70, 58, 44, 35))
                                for i in range(3000)]
    add("cl_flat4", dw.Deflate().dynamic(True, ll15, dl15, tokens, cl_lens=[4] * 16 + [0] * 3), tokens)
    # a 16-run that starts in the last literal / length lengths and goes on into the distance lengths
    ll = [8] * 166 + [9] * 116 + [5] * 4
    dl = [5] * 28 + [4] * 2
    assert dw.kraft(ll) == 32768 and dw.kraft(dl) == 32768
    seq = dw.cl_runs(ll + dl)
    at, seam = 0, False
    for s, x in seq:
        rep = {16: 3 + x, 17: 3 + x, 18: 11 + x}.get(s, 1)
        seam |= s == 16 and at < 286 < at + rep
        at += rep
    tokens = [rng.randrange(256) for _ in range(100)]
    for _ in range(1500):
        tokens.append((rng.randint(3, 258), rng.randint(1, 100)) if rng.random() < 0.2 else rng.randrange(256))
    add("run16_across_the_seam", dw.Deflate().dynamic(True, ll, dl, tokens, runs=True), tokens, any_bytes=True, cover=dict(seam=seam))
    # zero runs of 138 (symbol 18 with all extra bits set) and nothing but 18s between the few codes
    ll = _lens([(A, 1), (256, 1)], 288)[:257]
    seq = dw.cl_runs(ll + [0])
    tokens = [A] * 777
    add("all_18_runs", dw.Deflate().dynamic(True, ll, [0], tokens, runs=True), tokens, cover=dict(full18=sum(1 for s, x in seq if s == 18 and x == 127)))
    return out


# ---- nested_gzip: real dynamic-block headers inside the stored blocks of an outer stream (gzip only; plain zlib)
def fastq_text(n_bytes, seed):
    rng = random.Random(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        rec = b"@read%07d/1\n%s\n+\n%s\n" % (i, bytes(rng.choices(b"ACGT", k=150)), bytes(rng.choices(b"FFFFFFF:,#", k=150)))
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)


def _nested_gzip():
    import zlib
    inner = gzip.compress(fastq_text(2_200_000, 5), 6, mtime=0)
    out = []
    for level in (0, 6):
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append(Case("nested_gzip_level%d" % level, "nested_gzip", z.compress(inner) + z.flush(), inner, any_bytes=True, gzip_only=True))
    return out


@functools.lru_cache(maxsize=None)
def legal():
    out = []
    for f in (_one_dist_code, _no_dist_code, _deep48, _random_codes, _dense, _first_group_sizes, _alt258, _tiny_blocks, _stored_extremes,
              _header_extremes, _nested_gzip):
        out += f()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def groups():
    g = {}
    for c in legal():
        g.setdefault(c.group, []).append(c)
    return g


# ---- rejected: streams damaged in exactly one named way each (text: what the member announces)
@functools.lru_cache(maxsize=None)
def rejected():
    out = []
    good_lit = _hlit(dw.balanced_lens({A, C, G, T, 256, 257, 258, 259}, 288))
    good_dist = [1, 1]
    base = [A, C, G, T] * 10
    text = dw.apply(base + [(4, 2)] + base)

    def add(name, d, cut=None):
        p = d.payload()
        out.append(Case("rejected_" + name, "rejected", p if cut is None else p[:cut], text))

    add("length_without_distance_code", dw.Deflate().dynamic(True, good_lit, [0], base + [("lsym", 258), ("raw", 0, 5)] + base))
    add("distance_beyond_the_start", dw.Deflate().dynamic(True, good_lit, _hdist(dw.lens_list({0: 1, 10: 1}, 32)), base + [(4, 45)] + base))
    add("fixed_distance_symbol_30", dw.Deflate().fixed(True, base + [("lsym", 258), ("dsym", 30)] + base))
    add("fixed_distance_symbol_31", dw.Deflate().fixed(True, base + [("lsym", 258), ("dsym", 31)] + base))
    add("fixed_symbol_286", dw.Deflate().fixed(True, base + [("lsym", 286)] + base))
    add("fixed_symbol_287", dw.Deflate().fixed(True, base + [("lsym", 287)] + base))
    over = list(good_lit)
    over[N] = 2  # eight codes of three bits and one of two
    add("oversubscribed_literal_code", dw.Deflate().dynamic(True, over, good_dist, base + [(4, 2)] + base))
    under = list(good_lit)
    under[259] = 0  # seven codes of three bits
    add("incomplete_literal_code", dw.Deflate().dynamic(True, _hlit(under), good_dist, base + [(4, 2)] + base))
    noeob = list(good_lit)
    noeob[256], noeob[N] = 0, 3
    add("no_end_of_block_code", dw.Deflate().dynamic(True, noeob, good_dist, base + [(4, 2)] + base, eob=False))
    seq = dw.cl_plain(good_lit + good_dist)
    cl = dw.balanced_lens({s for s, _ in seq} | {16, 18}, 19)
    add("run_16_first", dw.Deflate().dynamic(True, good_lit, good_dist, base, cl_lens=cl, cl_seq=[(16, 0)] + seq[3:]))
    add("run_past_the_lengths", dw.Deflate().dynamic(True, good_lit, good_dist, base, cl_lens=cl, cl_seq=seq[:-2] + [(18, 0)]))
    wide = dw.balanced_lens({A, C, G, T, 256, 257, 258, 286}, 288)[:287]  # HLIT field 30: 287 codes
    add("hlit_287", dw.Deflate().dynamic(True, wide, good_dist, base))
    add("len_nlen_mismatch", dw.Deflate().fixed(False, base).stored(True, bytes(base), nlen=len(base) ^ 0xfffe))
    d = dw.Deflate().fixed(False, base)
    d.bits(1, 1)
    d.bits(3, 2)
    d.bits(0, 32)
    add("btype_3", d)
    d = dw.Deflate().dynamic(True, good_lit, good_dist, base + [(4, 2)] + base)
    add("ends_inside_a_token", d, cut=len(d.payload()) - 6)
    return tuple(out)
