"""gs_asmsum on the device, held to tests/asmsum.py: the hand-worked cases, each either judged or refused at the right line; chunk
sizes where the scans change shape; judged tabs on either side of a tile edge; the line limit; refusal and append; the cap."""
import numpy as np
import pytest

import asmsum
import genestrip_amd as ga
from asmsum_cases import CAP_CASES, CASES, KNOWN, cfg_of, rec

pytestmark = pytest.mark.gpu

TILE = 4096


def _handle(c, reserve_entries=0):
    flt = None
    if c["filter"] is not None:
        flt = np.zeros(len(c["known"]), dtype=np.uint8)
        flt[sorted(c["filter"])] = 1
    q = None if c["quality_mask"] == -1 else [i for i in range(11) if c["quality_mask"] >> i & 1]
    return ga.DeviceAssemblySummary(c["known"], filter=flt, qualities=q, reference_only=c["reference_only"], use_species_taxid=c["use_species_taxid"],
                                    device=0, reserve_entries=reserve_entries)


def _run(chunks, c, max_per_node=0, reserve_entries=0, last=True):
    """the chunks of one stream through a handle; a refused chunk goes through asmsum.py and is appended -> (picks, info, reports)"""
    reports, first_line = [], 0
    with _handle(c, reserve_entries) as h:
        for i, chunk in enumerate(chunks):
            ends = last and i == len(chunks) - 1
            r = h.submit(chunk, last=ends)
            assert r["refused"] == (asmsum.in_grammar(chunk, c, last=ends) >= 0) and r["first_bad_line"] == asmsum.in_grammar(chunk, c, last=ends)
            n_lines = len(asmsum.lines_of(chunk))
            if r["refused"]:
                assert (r["counted"], r["kept"], r["short"]) == (0, 0, 0)
                entries, counted, _, _ = asmsum.relevant_entries(chunk, c, first_line)
                h.append(entries, n_counted=counted, n_lines=n_lines)
            else:
                entries, counted, short, skipped = asmsum.relevant_entries(chunk, c)
                assert (r["counted"], r["kept"], r["short"], r["skipped"]) == (counted, len(entries), short, skipped), r
                assert r["pool_bytes"] == sum(len(e[1]) + len(e[2]) + len(e[3]) for e in entries)
                parts = chunk.split(b"\n")
                assert r["longest_line"] == max([len(x) + 1 for x in parts[:-1]] + [len(parts[-1])])
            reports.append(r)
            first_line += n_lines
        info = h.finish(max_per_node)
        return h.fetch(), info, reports


def _check_stream(chunks, c, max_per_node=0, **kw):
    text = b"".join(chunks)
    entries, counted, _, _ = asmsum.relevant_entries(text, c)
    want = asmsum.cap(entries, max_per_node)
    picks, info, reports = _run(chunks, c, max_per_node, **kw)
    assert picks == want
    assert info == (len(entries), len(want), len({e[0] for e in entries}), counted)
    return entries, want, reports


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked_cases(name):
    text, _, entries, counted, short, skipped, throws, device = CASES[name]
    c = cfg_of(name)
    with _handle(c) as h:
        r = h.submit(text, last=True)
        assert r["first_bad_line"] == device and r["refused"] == (device >= 0)
        if device >= 0:
            assert (r["counted"], r["kept"], r["short"], r["pool_bytes"]) == (0, 0, 0, 0)
            if throws is None:
                h.append(entries, n_counted=counted, n_lines=counted + short + skipped)
        else:
            assert (r["counted"], r["kept"], r["short"], r["skipped"]) == (counted, len(entries), short, skipped)
        if throws is None:
            assert h.finish(0) == (len(entries), len(entries), len({e[0] for e in entries}), counted)
            assert h.fetch() == asmsum.cap(entries, 0)


def _filler(n):
    """n bytes of comment lines (and, for one byte, an empty line)"""
    out = b""
    while n > 0:
        k = min(n, 2000)
        out += b"#" * (k - 1) + b"\n"
        n -= k
    return out


@pytest.fixture(scope="module")
def generated():
    known = sorted({7, 562, 9606, 10090} | {1000 + 13 * i for i in range(40)})
    return known, asmsum.summary(14000, known, seed=31)  # about 1100 tiles


def test_chunks_of_no_and_one_byte():
    c = asmsum.cfg(KNOWN)
    for chunk in (b"", b"x", b"\n", b"\t", b"#"):
        picks, info, reports = _run([chunk], c)
        assert picks == [] and info[:3] == (0, 0, 0) and not reports[0]["refused"]
    with _handle(c) as h:
        assert h.submit(b"x", last=False)["first_bad_line"] == 0  # an unterminated tail inside the stream


@pytest.mark.parametrize("n_bytes", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 1024 * TILE, 1025 * TILE + 7])
def test_chunk_sizes_where_the_scans_change_shape(generated, n_bytes):
    """one tile, two tiles, and 1024 / 1025 tiles: where the scan over the tile sums gives a thread two of them"""
    known, text = generated
    assert len(text) > n_bytes
    cut = text[:n_bytes]
    chunk = cut[:cut.rfind(b"\n") + 1]
    chunk += _filler(n_bytes - len(chunk))  # (a comment line makes it the size)
    assert len(chunk) == n_bytes
    entries, want, _ = _check_stream([chunk], asmsum.cfg(known, quality_mask=-1), max_per_node=2)
    assert len(entries) > 0 and (len(entries) > len(want) or n_bytes < 3 * TILE)


def test_more_line_blocks_than_scan_threads():
    """1025 blocks of 256 lines: the scan over the line blocks gives a thread two of them; tiles of nothing but newlines among them"""
    c = asmsum.cfg(KNOWN, quality_mask=-1)
    text = b"\n" * (1024 * 256) + rec() + b"\n" + b"\n" * 300 + rec(taxid=b"7") + b"\n"
    entries, _, reports = _check_stream([text], c)
    assert [e[6] for e in entries] == [1024 * 256, 1024 * 256 + 301] and reports[0]["skipped"] == 1024 * 256 + 300


def test_a_tile_of_newlines_and_a_tile_of_tabs():
    c = asmsum.cfg(KNOWN, quality_mask=-1)
    tabs = (b"\t" * 19 + b"\n") * 300  # 20 empty fields each: counted, no node
    text = rec() + b"\n" + b"\n" * (2 * TILE) + rec(taxid=b"7") + b"\n" + tabs + rec(taxid=b"9606") + b"\n"
    entries, _, reports = _check_stream([text], c)
    assert len(entries) == 3 and reports[0]["counted"] == 303


TABS = (4, 5, 6, 7, 10, 11, 12, 19, 20)


@pytest.mark.parametrize("tab", TABS)
def test_judged_tabs_on_either_side_of_a_tile_edge(tab):
    c = asmsum.cfg(KNOWN, quality_mask=-1)
    line = rec(cat=b"reference genome", taxid=b"10090", species=b"7", level=b"Scaffold")
    pos = [i for i, b in enumerate(line) if b == 9][tab - 1]
    for tile in (1, 2):
        for at in (tile * TILE - 1, tile * TILE):  # the tab is the tile's last byte, or the next tile's first
            start = at - pos
            text = _filler(start) + line + b"\n" + rec() + b"\n"
            assert text[at] == 9 and text.count(b"\t", start, at) == tab - 1
            entries, _, _ = _check_stream([text], c)
            assert [(e[0], e[4], e[5]) for e in entries] == [(3, 5, True), (1, 1, False)]
            entries, _, _ = _check_stream([text], asmsum.cfg(KNOWN, quality_mask=-1, use_species_taxid=True))
            assert [(e[0], e[1], e[2]) for e in entries] == [(0, b"10090", b"7"), (1, b"562", b"562")]


def test_a_line_that_ends_at_a_tile_edge_and_the_line_limit():
    c = asmsum.cfg(KNOWN)
    fits = rec(organism=b"o" * (TILE - 1 - len(rec(organism=b""))))  # TILE bytes with its newline
    assert len(fits) + 1 == TILE == asmsum.MAX_LINE
    entries, _, reports = _check_stream([fits + b"\n" + rec(taxid=b"7") + b"\n"], c)
    assert len(entries) == 2 and reports[0]["longest_line"] == TILE
    entries, _, _ = _check_stream([b"#\n" + fits + b"\n" + fits + b"\n" + fits], c)  # ... at every offset of the edge, and as the tail
    assert len(entries) == 3
    over = rec(organism=b"o" * (TILE - len(rec(organism=b""))))
    for text, bad in ((rec() + b"\n" + over + b"\n" + rec() + b"\n", 1), (over + b"\n", 0), (rec() + b"\n" + fits + b"xx", 1),
                      (b"\n" + rec(organism=b"o" * 3 * TILE) + b"\n", 1), (b"#" * (5 * TILE), 0)):
        with _handle(c) as h:
            r = h.submit(text, last=True)
            assert r["refused"] == 1 and r["first_bad_line"] == bad == asmsum.in_grammar(text, c, last=True)
            assert h.finish(1)[:2] == (0, 0)


def _split(text, n):
    lines = text.split(b"\n")[:-1]
    step = len(lines) // n + 1
    return [b"".join(x + b"\n" for x in lines[i:i + step]) for i in range(0, len(lines), step)]


def test_several_chunks_equal_one_stream(generated):
    known, text = generated
    text = text[:text.rfind(b"\n", 0, 40 * TILE) + 1]
    c = asmsum.cfg(known)
    one, _, _ = _check_stream([text], c, max_per_node=1)
    for reserve in (0, 100000):
        several, want, _ = _check_stream(_split(text, 5), c, max_per_node=1, reserve_entries=reserve)
        assert several == one
    assert len(one) > 40 and len(one) - len(want) > 10


def test_a_refused_chunk_leaves_the_handle_untouched(generated):
    known, text = generated
    a, b, d = _split(text[:text.rfind(b"\n", 0, 30 * TILE) + 1], 3)
    c = asmsum.cfg(known, quality_mask=-1)
    for bad in (b.replace(b"\n", b"\r\n", 1), b + rec(taxid=b"\xc4\xb1000") + b"\n", b + rec(organism=b"o" * TILE) + b"\n"):
        with _handle(c) as h:  # behind the refusal the handle is what it was behind a
            h.submit(a)
            r = h.submit(bad)
            assert r["refused"] == 1 and (r["counted"], r["kept"], r["short"], r["pool_bytes"]) == (0, 0, 0, 0)
            entries, counted, _, _ = asmsum.relevant_entries(a, c)
            assert h.finish(0) == (len(entries), len(entries), len({e[0] for e in entries}), counted)
            assert h.fetch() == asmsum.cap(entries, 0)
        _check_stream([a, bad, d], c, max_per_node=2, last=False)  # the parser's entries in its place give the stream's result


def test_device_text_and_state_rules(generated):
    torch = pytest.importorskip("torch")
    known, text = generated
    text = text[:text.rfind(b"\n", 0, 9 * TILE) + 1]
    c = asmsum.cfg(known, quality_mask=-1)
    entries, counted, _, _ = asmsum.relevant_entries(text, c)
    with _handle(c) as h:
        with pytest.raises(ga.GsError) as e:
            h.fetch()
        assert e.value.code == -5
        r = h.submit(torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda())
        assert (r["counted"], r["kept"]) == (counted, len(entries))
        h.kernel_time(True)
        assert h.finish(0)[0] == len(entries) and h.fetch() == asmsum.cap(entries, 0)
        assert h.kernel_time()[0] > 0
        for call in (lambda: h.submit(b"x\n"), lambda: h.append([]), lambda: h.finish(1)):
            with pytest.raises(ga.GsError) as e:
                call()
            assert e.value.code == -5


@pytest.mark.parametrize("case", range(len(CAP_CASES)))
def test_cap_cases(case):
    qualities, max_per_node, left = CAP_CASES[case]
    levels = {1: (b"Complete Genome", b"latest"), 2: (b"Complete Genome", b"x"), 3: (b"Chromosome", b"latest"), 7: (b"Contig", b"latest"), 9: (b"", b"latest")}
    text = b"".join(rec(level=levels[q][0], status=levels[q][1], ftp=b"f%d" % i) + b"\n" for i, q in enumerate(qualities))
    _, want, _ = _check_stream([text], asmsum.cfg(KNOWN, quality_mask=-1), max_per_node=max_per_node)
    assert [e[6] for e in want] == left


def test_the_cap_over_many_entries_and_many_nodes():
    known = list(range(1, 3001))
    rows = [rec(taxid=b"%d" % (1 + i), level=b"Contig") for i in range(0, 3000, 2)]  # many nodes with one entry, node 0 among them
    levels = [b"Complete Genome", b"Chromosome", b"Scaffold", b"Contig", b"x"]
    rows += [rec(taxid=b"1500", level=levels[i * 7 % 5], status=b"latest" if i % 3 else b"old", ftp=b"big%d" % i) for i in range(700)]  # more than a block has threads
    rows += [rec(taxid=b"3000", level=levels[i % 2], ftp=b"last%d" % i) for i in range(5)]  # node n_nodes - 1, ties at the cut
    rows += [rec(taxid=b"1", level=b"Chromosome", ftp=b"first%d" % i) for i in range(3)]  # node 0 again
    text = b"".join(r + b"\n" for r in rows)
    for max_per_node in (1, 2, 300, 700, 0):
        entries, want, _ = _check_stream(_split(text, 3), asmsum.cfg(known, quality_mask=-1), max_per_node=max_per_node, last=False)
        assert len(entries) == len(rows)
    entries, want, _ = _check_stream([text], asmsum.cfg(known, quality_mask=-1, filter={1499}), max_per_node=3)  # a filter of one node
    assert len(entries) == 700 and len(want) == 3
