"""tests/chunkscale.py on its own: the reference of the four-line cut against a byte-by-byte loop, and every builder of a large text
for the properties tests/test_gpu_chunk_scale.py relies on -- line, record and tile counts beyond the steps of the block scans, a
newline in every thread's run of tiles, output beyond the copy grid of a given number of compute units.  No device."""
import numpy as np
import pytest

import chunkscale as cs
import recordtext as rt
import streamgoals as sg


def test_cut_reference_against_a_plain_loop():
    rng = np.random.default_rng(1)
    texts = [b"", b"\n", b"A", b"\n\n\n", b"\n\n\n\n", b"\n\n\n\nA", b"a\nb\nc\nd\ne\n", b"a\nb\nc\nd\ne\nf\ng\nh", b"A" * 50]
    for _ in range(40):
        n = int(rng.integers(1, 60))
        texts.append(bytes(rng.choice(np.frombuffer(b"AC\n", dtype=np.uint8), n, p=[0.4, 0.3, 0.3])))
    for t in texts:
        assert cs.cut_reference(t) == cs.cut_loop(t), t
        assert cs.cut_reference(np.frombuffer(t, dtype=np.uint8)) == cs.cut_loop(t)
    assert cs.cut_reference(b"a\nb\nc\nd\ne\n") == (4, 8) and cs.cut_reference(b"\n\n\n") == (0, 0)


def test_small_cut_cases_hold_what_their_names_say():
    cases = cs.small_cut_cases()
    for name, text in cases.items():
        assert cs.cut_reference(text) == cs.cut_loop(text), name
    want = {"length 0": (0, 0), "length 1": (0, 0), "0 newlines": (0, 0), "3 newlines": (0, 0), "4 newlines": (4, 5001), "7 newlines": (4, 5001),
            "target first byte of a tile": (None, 2 * cs.TILE + 1), "target last byte of a tile": (None, 2 * cs.TILE),
            "four newlines open the text": (4, 4), "target last byte of the text": (None, 2 * cs.TILE + 77),
            "target in tile 15 of 40": (None, 15 * cs.TILE + 778), "target in tile 16 of 40": (None, 16 * cs.TILE + 778),
            "target in tile 39 of 40": (None, 39 * cs.TILE + 778), "target last byte of tile 15": (None, 16 * cs.TILE),
            "target first byte of tile 16": (None, 16 * cs.TILE + 1), "target behind 30 empty tiles": (4, 30 * cs.TILE + 2001),
            "a tile of newlines": (cs.TILE, 2 * cs.TILE), "only newlines": (2 * cs.TILE, 2 * cs.TILE)}
    for name, (n_lines, cut) in want.items():
        got = cs.cut_reference(cases[name])
        assert got[1] == cut and (n_lines is None or got[0] == n_lines), (name, got)
    for n in (15, 17, 4095, 4097, 5 * cs.TILE + 1234):  # a newline in the bytes behind the last whole 16-byte word
        t = cases["length %d" % n]
        assert n % 16 and t[-1] == cs.NL and (t[n & ~15:] == cs.NL).any()
    assert len(cases["5 newlines"]) == 10000 and cases["5 newlines"][-1] != cs.NL
    counts = cs.tile_counts(cases["another count in every tile"].tobytes())
    assert counts.tolist() == list(range(1, 51))
    assert cs.tile_run(40) == 16  # tiles 15 and 16 lie on either side of the edge between the first two threads' runs


@pytest.mark.parametrize("n_tiles", [cs.STEP_TILES, cs.STEP_TILES + 1, cs.STEP_TILES + 16 * 3 + 5])
def test_step_cut_cases(n_tiles):
    n, per = cs.step_cut_bytes(n_tiles), cs.tile_run(n_tiles)
    assert cs.tiles(n) == n_tiles and per == (16 if n_tiles == cs.STEP_TILES else 32)
    owned = n_tiles - (n_tiles - 1) // per * per  # tiles of the last thread that owns any
    assert owned == {cs.STEP_TILES: 16, cs.STEP_TILES + 1: 1, cs.STEP_TILES + 53: 21}[n_tiles]
    seen = set()
    for what, pos in cs.step_cut_cases(n_tiles):
        after = len(pos) % 4
        target = int(pos[len(pos) - after - 1])
        seen.add(target // cs.TILE // per)
        assert pos[-1] < n and len(np.unique(pos)) == len(pos), what
        if what in ("tile 31", "tile 32"):
            assert target // cs.TILE == int(what[5:])
    assert {0, n_tiles // 2 // per, (n_tiles - 1) // per} <= seen
    what, pos = cs.step_cut_cases(n_tiles)[3]
    text = cs.newline_text(n, pos)
    assert cs.cut_reference(text) == (len(pos) & ~3, int(pos[(len(pos) & ~3) - 1]) + 1) and cs.tiles(cs.cut_reference(text)[1]) == n_tiles


def test_short_records():
    n = 1024 * cs.BLOCK + 5
    text, recs, reads = cs.short_records(n)
    assert cs.block_run(n) == 2 and cs.block_run(2 * 1024 * cs.BLOCK + 257) == 3
    assert text.count(b"\n") == 4 * n and len(recs) == n and len(text) < 30 * n
    assert text.endswith(b"\n".join((recs[-1][0], recs[-1][1], b"+", recs[-1][3])) + b"\n") and recs[-1][0].startswith(b"@s-last/")
    assert sum(d.startswith(b"@s1/") for d, _, _, _ in recs[:cs.BLOCK]) in (85, 86)  # a third of every block
    assert {len(r) for r in reads} == set(range(1, 9)) and len(reads) == cs.SHORT_CYCLE
    head = text[:text.index(b"@s1/4 ")]
    assert sg.extract(head, b"s1/")[0] == b"".join(b"%s\n%s\n+\n%s\n" % (d, s, q) for d, s, _, q in recs[:4] if d.startswith(b"@s1/"))


@pytest.mark.parametrize("n_cu", [256, 304])
def test_fasta_text(n_cu):
    text = cs.fasta_text(n_cu)
    t = np.frombuffer(text, dtype=np.uint8)
    nl = np.flatnonzero(t == cs.NL)
    starts = np.concatenate(([0], nl[:-1] + 1))
    n_lines, n_records = len(nl), int((t[starts] == ord(">")).sum())
    assert text.endswith(b"\n") and n_lines > 2 * 1024 * cs.BLOCK and cs.block_run(n_lines) == 3
    assert n_records == 2 * 140_000 + 2 > 1024 * cs.BLOCK and cs.block_run(n_records) == 2
    lens = np.diff(np.concatenate(([-1], nl)))
    assert int(lens.max()) == 60_000 < cs.LONG_LINE and int((lens == 60_000).sum()) == 1
    at = text.index(b">sL ")
    long = text[at:text.index(b">sS ")]
    assert len(long) - long.count(b"\n") > cs.copy_grid_bytes(n_cu) + (1 << 20)  # its bases alone span the copy grid


def test_fasta_text_with_crlf_and_empty_lines():
    plain, crlf = cs.fasta_text(4, n_small=300), cs.fasta_text(4, n_small=300, crlf=True)
    assert b"\r\n\r\n" in crlf and b"\n\n" in crlf and b"\r\r\n" in crlf and crlf.count(b"\r\n") > plain.count(b"\n")
    (got, n), want = sg.fasta2fastq(crlf), sg.fasta2fastq(crlf.replace(b"\r", b""))  # (the goal keeps the '\r' of a header line, and of no other)
    assert (got.replace(b"\r\n", b"\n"), n) == want and got.count(b"\r") == n == sg.fasta2fastq(plain)[1]


def test_fastq_ml_records():
    n = 60_000
    recs = cs.fastq_ml_records(n)
    text = rt.fastq_ml(recs)
    assert text.count(b"\n") > 1024 * cs.BLOCK and cs.block_run(text.count(b"\n")) == 2
    assert {r[3] for r in recs} == {2, 3} and {r[4] for r in recs} == {1, 2, 3} and any(len(q) > len(s) for _, s, q, _, _ in recs)
    few = rt.fastq_ml(recs[:200])
    ents = rt.entries(few, False)
    assert [(d, s, q) for d, s, q in ents] == [(d, s, q) for d, s, q, _, _ in recs[:200]]
    assert sum(s[:2] in (b"AC", b"AT") and s == s[:2] * (len(s) // 2) for _, s, _, _, _ in recs[:200]) >= 40


@pytest.mark.parametrize("n_tiles", [cs.STEP_TILES + 1])
def test_wide_chunk(n_tiles):
    n = n_tiles * cs.TILE - 1000
    text = cs.wide_chunk(n)
    assert len(text) == n and cs.tiles(n) == n_tiles and text.endswith(b"\n") and text.count(b"\n") % 4 == 0
    counts = cs.tile_counts(text)
    runs = np.add.reduceat(counts, np.arange(0, n_tiles, 16))
    assert (runs > 0).all()  # every 16-tile run holds a newline: a slip in any thread's sum moves nl[]
    assert counts.max() > 500 and counts[-1] > 0
    empty = np.flatnonzero(counts == 0)
    assert len(empty) and max(len(r) for r in np.split(empty, np.flatnonzero(np.diff(empty) > 1) + 1)) >= 3  # (a line of 20 000 bytes)
    head = text[:200_000]
    head = head[:head.rindex(b"\n@w") + 1]
    out, k = sg.extract(head, b"w1/")
    assert 0 < k < head.count(b"\n") // 4 and abs(3 * k - head.count(b"\n") // 4) <= 3


def test_wide_chunk_sizes_are_exact():
    for n in (70_001, 70_002, 200_000, 300 * cs.TILE + 1):
        assert len(cs.wide_chunk(n)) == n


def test_deflate_text():
    for n in (1025 * 16384 + 1, 2049 * 16384 + 7):
        t = cs.deflate_text(n)
        assert len(t) == n and t.startswith(b"@r000000000\n") and t.count(b"\n+\n") > n // 250
    import zlib
    piece = lambda i: len(zlib.compress(t[i * 16384:(i + 1) * 16384], 1))
    assert piece(n // 3 // 16384 + 2) > 2 * piece(5)  # the random stretch: members of very different sizes
