"""Builders of the large texts of tests/test_gpu_chunk_scale.py, and the plain reference of the four-line cut.  A helper module of
the suite, not a test file, and independent of the library: nothing here calls it.  tests/test_chunk_scale_cpu.py checks every
builder for the properties the GPU tests rely on.

Every text stage finds its offsets with a two-level prefix sum: blocks of BLOCK items scanned in place, the per-block sums scanned by
ONE block of SCAN_THREADS threads.  Up to SCAN_THREADS sums a thread owns one of them, beyond that a run of `per`; the texts built
here are the smallest ones that take the kernels beyond that step."""
import numpy as np

TILE = 4096          # GS_TEXT_TILE (gs_text.hip); the tile of gi_count_kernel (gs_inflate_dev.hip: tile * 4096)
BLOCK = 256          # GS_SCAN_BLOCK (gs_scan.h) = RW_BLOCK = KR_BLOCK; GS_FA_BLOCK (gs_text.hip); GC_BLOCK (gs_deflate_dev.hip)
SCAN_THREADS = 1024  # __launch_bounds__(1024) of gs_text_scan_kernel, gi_cut_kernel, gs_fasta_scan_kernel, rw_scan_kernel, gc_scan_kernel, gd_offsets_kernel
COPY_PIECE = 4096    # RW_PIECE = RW_BLOCK * 16 (gs_rewrite.hip)
COPY_BLOCKS_PER_CU = 8  # gs_launch_rewrite_copy: grid = min(pieces, n_cu * 8)
LONG_LINE = 65534    # RW_LONG_LINE (gs_rewrite.hip)
STEP_TILES = 16 * SCAN_THREADS  # tiles up to which a thread of the tile scans owns 16 counts

NL = 10
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def tiles(n_bytes):
    return (n_bytes + TILE - 1) // TILE


def tile_run(n_tiles):
    """tile counts per thread of gs_text_scan_kernel and gi_cut_kernel: per = ((n_tiles + 1023) / 1024 + 15) & ~15"""
    return ((n_tiles + SCAN_THREADS - 1) // SCAN_THREADS + 15) & ~15


def block_run(n_items):
    """block sums per thread of the scans over blocks of BLOCK items: per = (n_blocks + 1023) / 1024"""
    n_blocks = (n_items + BLOCK - 1) // BLOCK
    return (n_blocks + SCAN_THREADS - 1) // SCAN_THREADS


def copy_grid_bytes(n_cu):
    """output bytes from which the blocks of rw_copy_kernel take more than one piece each"""
    return n_cu * COPY_BLOCKS_PER_CU * COPY_PIECE


# ---- the four-line cut ----
def cut_reference(text):
    """(n_lines, cut) of gs_text_cut_device: the newlines of the whole four-line records, and the bytes up to and including the
    last of them"""
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == NL if isinstance(text, (bytes, bytearray)) else text == NL)
    n_lines = len(nl) & ~3
    return n_lines, (int(nl[n_lines - 1]) + 1 if n_lines else 0)


def cut_loop(text):
    """the same, byte by byte"""
    seen, cut = 0, 0
    for i, b in enumerate(bytes(text)):
        if b == NL:
            seen += 1
            if seen % 4 == 0:
                cut = i + 1
    return seen - seen % 4, cut


def newline_text(n, positions):
    """n bytes of 'A' with newlines at `positions`"""
    t = np.full(n, ord("A"), dtype=np.uint8)
    if len(positions):
        t[np.asarray(positions, dtype=np.int64)] = NL
    return t


def cut_positions(n, target, after=0, background=True):
    """newline positions in n bytes so that the newline at byte `target` is the last one whose number is a multiple of four:
    background newlines in the tiles in front of the target's (tile t holds t % 3 of them), up to three more right in front of the
    target to make its number a multiple of four, and `after` (0 .. 3) newlines between the target and the last byte"""
    assert 3 <= target < n and 0 <= after <= 3
    pos = set()
    if background:
        for t in range(target // TILE):
            pos.update(t * TILE + 17 + 5 * j for j in range(t % 3))
    pos.discard(target)
    p = target - 1
    while (len(pos) + 1) % 4:
        assert p >= 0
        if p not in pos:
            pos.add(p)
        p -= 1
    pos.add(target)
    assert n - 1 - target >= after
    pos.update(target + (n - 1 - target) * (j + 1) // after for j in range(after))
    out = np.array(sorted(pos), dtype=np.int64)
    assert len(out) - after == np.searchsorted(out, target) + 1 and (len(out) - after) % 4 == 0
    return out


def small_cut_cases():
    """name -> text (numpy uint8): the shapes of one and a few tiles"""
    cases = {}
    # lengths: newlines down to the last byte, so that the tail a thread of gi_count_kernel reads byte by byte holds some
    for n in (0, 1, 15, 16, 17, 4095, 4096, 4097, 5 * TILE + 1234):
        cases["length %d" % n] = newline_text(n, sorted(set(range(3, n, 5)) | ({n - 1} if n else set())))
    spread = [100, 4095, 4096, 5000, 8191, 8192, 9000]
    for k in range(8):  # 0 .. 3: no record; 4: one; 5 .. 7: the cut steps back to the fourth.  The text does not end in a newline
        cases["%d newlines" % k] = newline_text(10000, spread[:k])
    cases["no newline in 3 tiles and a byte"] = newline_text(3 * TILE + 1, [])
    # the last fourth-multiple newline at the edges of a tile and of the text (byte 3 is the first byte that can hold it)
    cases["target first byte of a tile"] = newline_text(3 * TILE + 50, cut_positions(3 * TILE + 50, 2 * TILE, after=2))
    cases["target last byte of a tile"] = newline_text(3 * TILE + 50, cut_positions(3 * TILE + 50, 2 * TILE - 1, after=3))
    cases["four newlines open the text"] = newline_text(2 * TILE, [0, 1, 2, 3, 5000])
    cases["target last byte of the text"] = newline_text(2 * TILE + 77, cut_positions(2 * TILE + 77, 2 * TILE + 76))
    # the edge between the runs of thread 0 and thread 1 at per = 16, the last tile, a target behind tiles without a newline
    n = 40 * TILE - 100
    for tile in (15, 16, 39):
        cases["target in tile %d of 40" % tile] = newline_text(n, cut_positions(n, tile * TILE + 777, after=tile % 3 if tile < 39 else 0))
    cases["target last byte of tile 15"] = newline_text(n, cut_positions(n, 16 * TILE - 1, after=1))
    cases["target first byte of tile 16"] = newline_text(n, cut_positions(n, 16 * TILE, after=1))
    cases["target behind 30 empty tiles"] = newline_text(n, [5, 6, 7, 30 * TILE + 2000, 39 * TILE])
    # dense tiles
    cases["a tile of newlines"] = newline_text(3 * TILE, list(range(TILE, 2 * TILE)) + [2 * TILE + 9, 3 * TILE - 1])
    cases["only newlines"] = newline_text(2 * TILE + 3, range(2 * TILE + 3))
    cases["another count in every tile"] = newline_text(50 * TILE - 3, [t * TILE + 3 * j for t in range(50) for j in range(t + 1)])
    return cases


def step_cut_cases(n_tiles):
    """[(what, newline positions)] for a text of n_tiles tiles (step_cut_bytes): the target in the first thread's run, in a middle
    run, at both ends of the last run that is not empty, and on either side of the run edge behind tile 31"""
    n, per = step_cut_bytes(n_tiles), tile_run(n_tiles)
    last_run = (n_tiles - 1) // per * per
    spots = [("first run", 5), ("middle run", n_tiles // 2), ("start of the last run", last_run), ("last tile", n_tiles - 1), ("tile 31", 31), ("tile 32", 32)]
    return [(what, cut_positions(n, min(tile * TILE + 1000 + 3 * i, n - 1), after=i % 4)) for i, (what, tile) in enumerate(spots)]


def step_cut_bytes(n_tiles):
    """a text of n_tiles tiles whose last tile is cut short in the middle of a 16-byte word (a whole last tile at STEP_TILES)"""
    return n_tiles * TILE - (0 if n_tiles == STEP_TILES else 1029)


def tile_counts(text):
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == NL)
    return np.bincount(nl // TILE, minlength=tiles(len(text)))


# ---- four-line chunks of short records ----
def _cycle(n, lo, hi, seed):
    """n reads of lo .. hi bases (those of four bases and more distinct) with a quality line each"""
    rng = np.random.default_rng(seed)
    reads, seen = [], set()
    while len(reads) < n:
        r = ACGT[rng.integers(0, 4, int(rng.integers(lo, hi + 1)))].tobytes()
        if len(r) >= 4 and r in seen:
            continue
        seen.add(r)
        reads.append(r)
    quals = [bytes(b"IJKL#5"[x] for x in rng.integers(0, 6, len(r))) for r in reads]
    return reads, quals


SHORT_CYCLE = 331  # distinct reads of a chunk of short records (a prime: no period shared with the blocks of 256)


def short_records(n, seed=1):
    """n four-line records of about 26 bytes: descriptors '@s<i % 3>/<i> x', the last one '@s-last/<i> x', reads of 1 .. 8 bases
    that repeat with period SHORT_CYCLE -> (text, [(descriptor, read, plus line, quality)], the reads of one period)"""
    reads, quals = _cycle(SHORT_CYCLE, 1, 8, seed)
    recs = [(b"@s%d/%d x" % (i % 3, i), reads[i % SHORT_CYCLE], b"+", quals[i % SHORT_CYCLE]) for i in range(n - 1)]
    recs.append((b"@s-last/%d x" % (n - 1), reads[(n - 1) % SHORT_CYCLE], b"+", quals[(n - 1) % SHORT_CYCLE]))
    text = b"".join(b"%s\n%s\n+\n%s\n" % (d, s, q) for d, s, _, q in recs)
    return text, recs, reads


# ---- FASTA beyond 262 144 lines and records, output beyond the copy grid ----
def _runs(n, lo, hi, seed):
    """n bases in runs of one base, lo .. hi long (few Kraken-style segments at any k), with a stretch of 600 random bases in the middle"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, n // lo + 1)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n)) + 1]
    s = np.repeat(ACGT[np.arange(len(lens)) % 4], lens)[:n].copy()
    assert len(s) == n
    if n > 2000:
        s[n // 2:n // 2 + 600] = ACGT[rng.integers(0, 4, 600)]
    return s.tobytes()


def fasta_text(n_cu, n_small=140_000, crlf=False):
    """FASTA text of: n_small records of 1 .. 7 bases ('>s<i % 9>/<i>'), one record of more than copy_grid_bytes(n_cu) bases in
    lines of 60 ('>sL ...'), one record of a single line of 60 000 bytes ('>sS ...'), n_small more small records.  crlf: CRLF line
    ends and a few empty lines (LF and CRLF) between records and inside the long one"""
    reads, _ = _cycle(SHORT_CYCLE, 1, 7, 5)
    eol = b"\r\n" if crlf else b"\n"
    small = lambda a, b: b"".join(b">s%d/%d%s%s%s" % (i % 9, i, eol, reads[i % SHORT_CYCLE], eol) for i in range(a, b))
    long = _runs(copy_grid_bytes(n_cu) + (1 << 20) + 7, 3000, 7000, 3)
    single = _runs(60_000 - len(eol), 200, 400, 4)
    assert len(single) + len(eol) == 60_000 < LONG_LINE
    lines = [long[i:i + 60] for i in range(0, len(long), 60)]
    if crlf:
        lines[1000:1000] = [b"", b"\r"]  # an empty line and one of a lone '\r' inside the long record
    gap = (b"\n\r\n" if crlf else b"")
    return b"".join([small(0, n_small), gap, b">sL chromosome one", eol, eol.join(lines), eol, gap, b">sS single line", eol, single, eol,
                     small(n_small, 2 * n_small), gap])


# ---- general FASTQ beyond 262 144 lines ----
def fastq_ml_records(n, seed=2):
    """[(descriptor line, sequence, quality, sequence lines, quality lines)] for recordtext.fastq_ml: reads of 20 .. 60 bases over
    2 .. 3 lines, qualities over 1 .. 3 lines, every seventh longer than its read; every fifth read is 'ACAC..' or 'ATAT..' (no
    k-mer of the k = 2 store of the tests)"""
    rng = np.random.default_rng(seed)
    pool = ACGT[rng.integers(0, 4, 1 << 16)].tobytes()
    qpool = bytes(b"IJKL#~5"[x] for x in rng.integers(0, 7, 1 << 12))
    recs = []
    for i in range(n):
        L = 20 + (i * 7) % 41
        o = (i * 131) % ((1 << 16) - 64)
        s = (b"AC" if i % 10 else b"AT") * (L // 2) if i % 5 == 0 else pool[o:o + L]
        qo = (i * 17) % ((1 << 12) - 80)
        recs.append((b"@K%d/%d ml" % (i % 3, i), s, qpool[qo:qo + len(s) + (3 if i % 7 == 0 else 0)], 2 + i % 2, 1 + i % 3))
    return recs


# ---- four-line chunks beyond 64 MiB ----
def wide_chunk(n_bytes, seed=7):
    """a four-line chunk of exactly n_bytes: records of about 2 KiB (reads of 1000 .. 1012 bases, descriptors '@w<i % 3>/<i> lane'),
    now and then a stretch of 300 records of 3 bases (hundreds of newlines in one tile) or a record of 40 KiB (tiles without any)"""
    rng = np.random.default_rng(seed)
    pool = ACGT[rng.integers(0, 4, 1 << 20)].tobytes()
    qpool = bytes(rng.integers(35, 74, 1 << 16, dtype=np.uint8))
    out, size, i = [], 0, 0

    def add(L):
        nonlocal size, i
        o, qo = (i * 7919) % ((1 << 20) - L), (i * 104729) % ((1 << 16) - 1100)
        q = qpool[qo:qo + L] if L <= 1100 else qpool[:20000] * (L // 20000 + 1)
        rec = b"@w%d/%d lane\n%s\n+\n%s\n" % (i % 3, i, pool[o:o + L], q[:L])
        out.append(rec)
        size += len(rec)
        i += 1

    while n_bytes - size > 64 * 1024:
        if i % 4000 == 1500:
            for _ in range(300):
                add(3)
        elif i % 5000 == 2500:
            add(20000)
        else:
            add(1000 + (i * 7) % 13)
    while n_bytes - size > 6000:
        add(1000 + (i * 7) % 13)
    desc = b"@w%d/%d lane" % (i % 3, i)
    rest = n_bytes - size - len(desc) - 5
    if rest % 2:
        desc, rest = desc + b"s", rest - 1
    L = rest // 2
    out.append(b"%s\n%s\n+\n%s\n" % (desc, pool[:L], qpool[:L]))
    text = b"".join(out)
    assert len(text) == n_bytes and L > 0
    return text


# ---- text for the deflate writer ----
def deflate_text(n_bytes, seed=3):
    """FASTQ-like text of exactly n_bytes with a stretch of 300 000 random bytes (members of very different sizes)"""
    rng = np.random.default_rng(seed)
    L = 100
    n = n_bytes // (2 * L + 16) + 1
    a = np.empty((n, 2 * L + 16), dtype=np.uint8)
    a[:, :3] = np.frombuffer(b"@r0", dtype=np.uint8)
    idx = np.arange(n, dtype=np.int64)
    for d in range(8):
        a[:, 10 - d] = (idx % 10 + 48).astype(np.uint8)
        idx //= 10
    a[:, 11] = NL
    a[:, 12:12 + L] = ACGT[rng.integers(0, 4, (n, L))]
    a[:, 12 + L:15 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    a[:, 15 + L:15 + 2 * L] = np.frombuffer(b"FFFFFFF:,#", dtype=np.uint8)[rng.integers(0, 10, (n, L))]
    a[:, 15 + 2 * L] = NL
    t = a.reshape(-1)[:n_bytes].copy()
    at = n_bytes // 3
    t[at:at + 300_000] = rng.integers(0, 256, 300_000, dtype=np.uint8)
    return t.tobytes()
