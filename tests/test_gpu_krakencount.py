"""The krakencount handle (gs_krakencount, genestrip_amd/csrc/gs_krakencount.hip) against the plain-Python restatement of the
reference (tests/krakencount.py): rows, totals, refusals, and the sizes at which its scans and its tables change shape."""
import numpy as np
import pytest

import genestrip_amd as ga
import krakencount as kc
from krakencount_cases import CASES, first_empty_line, line, long_line, random_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def counter():
    c = ga.KrakenCounter(0, max_taxids=1 << 13)
    yield c
    c.close()


@pytest.fixture(scope="module")
def geo(counter):
    return counter.geometry()


def device_rows(counter):
    ids, cnt = counter.fetch()
    return [(str(int(i)).encode(), int(c[0]), int(c[1]), int(c[2])) for i, c in zip(ids, cnt)]


def expect(chunks):
    """rows and totals of chunks that each are a stream of their own, into one table"""
    rows, tot = {}, [0, 0, 0, 0]
    for ch in chunks:
        r, t = kc.count(ch)
        for k, *v in r:
            rows[k] = [a + b for a, b in zip(rows.get(k, [0, 0, 0]), v)]
        tot = [a + b for a, b in zip(tot, (t["lines"], t["counted"], t["a_tokens"], t["long_lines"]))]
    return [(k, *rows[k]) for k in sorted(rows)], tuple(tot)


def check(counter, chunks):
    """a fresh table, the chunks one by one, all of them counted"""
    counter.reset()
    for ch in chunks:
        t = counter.submit(ch)
        rep = counter.chunk(t)
        assert rep["refused"] == 0, rep
    rows, tot = expect(chunks)
    assert device_rows(counter) == rows
    assert counter.status()[3] == tot
    assert counter.status()[0] == -1


GOOD_A = line(b"0:3 7:2 A:1", cls=b"7") + line(b"562:9", cls=b"0", flag=b"U")
GOOD_B = line(b"7:1 0:4", cls=b"562") * 3


def test_abi_and_geometry(counter, geo):
    assert ga.abi_version() == 3
    assert geo["scan_block_bytes"] == 4096 and geo["tile_bytes"] % geo["scan_block_bytes"] == 0
    assert geo["lds_slots"] >= 64 and geo["global_slots"] >= 2 * (1 << 13)
    assert geo["scan_levels"] == 3


@pytest.mark.parametrize("case", [c for c in CASES if c.bad_line is None and c.only is None], ids=lambda c: c.name)
def test_valid_cases(counter, case):
    counter.reset()
    rep = counter.chunk(counter.submit(case.data))
    assert rep["refused"] == 0
    assert device_rows(counter) == case.expect
    assert counter.status()[3][:3] == case.totals
    assert rep["first_empty_offset"] == first_empty_line(case.data)


@pytest.mark.parametrize("case", [c for c in CASES if c.bad_line is not None], ids=lambda c: c.name)
def test_refused_cases(counter, case):
    """outside the grammar: the chunk is refused with its first bad line, and the table is what the good chunks alone give"""
    counter.reset()
    assert counter.chunk(counter.submit(GOOD_A))["refused"] == 0
    t = counter.submit(GOOD_A + case.data)
    rep = counter.chunk(t)
    assert rep["refused"] == 1 and rep["first_bad_line"] == 2 + case.bad_line and rep["totals"] == (0, 0, 0, 0)
    assert device_rows(counter) == expect([GOOD_A])[0]
    assert counter.chunk(counter.submit(GOOD_B))["refused"] == 0
    rows, tot = expect([GOOD_A, GOOD_B])
    assert device_rows(counter) == rows
    ft, fb, _, totals = counter.status()
    assert (ft, fb, totals) == (t, 2 + case.bad_line, tot)


def test_refusals_outside_the_descriptor(counter):
    """bytes >= 0x80 are taken in the descriptor only; a blank in the descriptor refuses even without a ':'"""
    check(counter, [line(b"9:5", desc=b"r\xc3\xa4d")])
    for bad in (line(b"9:5", flag=b"\xc3"), line(b"9\xc3:5"), line(b"9:5", desc=b"a b"), line(b"9:5", cls=b"1234567890"), line(b"A7:5"),
                line(b"9:"), line(b":5"), line(b"9:05"), line(b" 9:5")):
        counter.reset()
        rep = counter.chunk(counter.submit(GOOD_A + bad + GOOD_A))
        assert rep["refused"] == 1 and rep["first_bad_line"] == 2, bad
        assert device_rows(counter) == []


def test_sizes_where_the_scans_change(counter, geo):
    """tile - 1, tile, tile + 1 bytes; one scan block and the first byte of a second (level 2); the first size at which a thread of
    the scan over the block sums owns more than one of them (level 3)"""
    rng = np.random.default_rng(11)
    tile, sb = geo["tile_bytes"], geo["scan_block_bytes"]
    for n in (64, sb - 1, sb, sb + 1, tile - 1, tile, tile + 1, 3 * tile + 17, (geo["level3_blocks"] - 1) * sb + 1):
        check(counter, [random_text(rng, n)])


@pytest.mark.parametrize("boundary", ["scan_block_bytes", "tile_bytes"])
def test_features_across_a_boundary(counter, geo, boundary):
    """the fourth tab, a 20-byte token and the newline of a line on every offset across the end of a scan block / of a tile"""
    rng = np.random.default_rng(5)
    b = geo[boundary]
    head = random_text(rng, b - 300)
    tail = random_text(rng, 400)
    probe = line(b"12345:678 A:5 999999999:999999999 7:1", cls=b"999999999", desc=b"")
    at = {"tab": probe.index(b"\t12345") , "token": probe.index(b"999999999:"), "newline": len(probe) - 1}
    chunks = []
    for what, off in at.items():
        for d in range(-24, 3):
            pad = 300 + d - off  # the feature lands on byte b + d
            chunks.append(head + probe[:2] + b"x" * pad + probe[2:] + tail)
            assert chunks[-1][b + d:b + d + 1] == probe[off:off + 1]
    check(counter, chunks)


def test_long_and_single_lines(counter, geo):
    tile = geo["tile_bytes"]
    one = long_line(2 * tile + 1000)  # one line longer than two tiles: a long line for the reference
    check(counter, [one])
    assert counter.status()[3][3] == 1
    check(counter, [line(b"9:1") + one + line(b"9:2 3:4", cls=b"3")])
    check(counter, [line(b"0:1")])
    check(counter, [line(b" ".join([b"A:%d" % i for i in range(3000)]), cls=b"0") * 2])  # 'A' tokens only
    assert device_rows(counter) == []
    check(counter, [long_line(65537)])
    assert counter.status()[3][3] == 1


def test_keyed_reduction(counter, geo):
    S = geo["lds_slots"]
    for n in (S - 1, S, S + 1, 4 * S):  # distinct tax ids in one tile: up to and beyond what a workgroup's table holds
        text = line(b" ".join(b"%d:%d" % (1000 + 3 * i, i % 7) for i in range(n)), cls=b"1000")
        assert len(text) <= geo["tile_bytes"]
        check(counter, [text, text])
    assert counter.counters()[1] > 0  # (4 * S keys: some tokens went straight to the global table)
    check(counter, [line(b" ".join([b"0:1"] * 100), cls=b"0") * 2000])  # 200 000 tokens on one key
    assert device_rows(counter) == [(b"0", 2000, 200000, 2000)]
    atomics, direct = counter.counters()
    assert direct == 0 and atomics <= 4 * (2000 * 401 // geo["tile_bytes"] + 1)  # a handful per workgroup, not one per token
    check(counter, [line(b"7:999999999", cls=b"7") * 5])
    assert device_rows(counter) == [(b"7", 5, 4999999995, 4999999995)]


def test_table_full():
    c = ga.KrakenCounter(0, max_taxids=4)
    try:
        a = line(b"1:1 2:2 3:3", cls=b"1")
        assert c.chunk(c.submit(a))["refused"] == 0
        over = line(b"1:1 4:1 5:1 6:1", cls=b"1")
        rep = c.chunk(c.submit(over))
        assert rep["refused"] == 2 and rep["rows"] == 3
        assert device_rows(c) == expect([a])[0]
        fits = line(b"2:5 4:1", cls=b"4")
        assert c.chunk(c.submit(fits))["refused"] == 0
        assert device_rows(c) == expect([a, fits])[0]
        assert c.chunk(c.submit(line(b"9:1")))["refused"] == 2
        assert device_rows(c) == expect([a, fits])[0]
        assert c.status()[0] == 1
    finally:
        c.close()


def test_several_chunks_and_reset(counter):
    rng = np.random.default_rng(3)
    chunks = [random_text(rng, n) for n in (5000, 70000, 300, 40000)]
    check(counter, chunks)
    assert device_rows(counter) == kc.count(b"".join(chunks))[0]  # no empty line: the chunks are one stream
    counter.submit(b"")
    assert device_rows(counter) == kc.count(b"".join(chunks))[0]
    counter.reset()
    assert device_rows(counter) == [] and counter.status() == (-1, -1, -1, (0, 0, 0, 0)) and counter.counters() == (0, 0)


def test_device_memory(counter):
    import torch

    text = random_text(np.random.default_rng(9), 50001)
    counter.reset()
    t = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    assert counter.chunk(counter.submit(t))["refused"] == 0
    assert device_rows(counter) == kc.count(text)[0]
    assert counter.kernel_time(True) == (0, 0.0)
    counter.submit(t)
    n, ms = counter.kernel_time(False)
    assert n == 1 and ms > 0
