"""The accession map handle (gs_accmap, genestrip_amd/csrc/gs_accmap.hip) against the plain-Python restatement of the reference
(tests/accmap.py): entries, order, counts, regions, refusals and lookups, at the sizes where the scan changes shape."""
import numpy as np
import pytest

import accmap
import genestrip_amd as ga
from accmap_cases import CASES, CFG, KNOWN, L, _sized, catalog, cfg_of

pytestmark = pytest.mark.gpu

TILE = 4096


def new_map(known=KNOWN, reserve=0, **over):
    cfg = dict(CFG)
    cfg.update(over)
    return ga.DeviceAccessionMap(known, cfg["categories"], cfg["statuses"], cfg["seq_type"], reserve_entries=reserve), cfg


def lines_of(text):
    return text.splitlines(keepends=True)


def filler(n):
    """exactly n bytes (0, or 6 and more) of lines inside the grammar that do not pass"""
    out = []
    while n >= 2012:
        out.append(b"x" * 994 + b"\t\t\t\t\t\n")
        n -= 1000
    if n:
        assert n >= 6
        out.append(b"x" * (n - 6) + b"\t\t\t\t\t\n")
    return b"".join(out)


def check(chunks, known=KNOWN, reserve=0, last=True, **over):
    """the chunks, whole lines inside the grammar each, into a fresh map: every report, the sorted entries, the counts and the regions
    are the restatement's over the chunks as one stream"""
    m, cfg = new_map(known, reserve, **over)
    try:
        entries, passing = [], 0
        for i, ch in enumerate(chunks):
            rep = m.submit(ch, last=last and i == len(chunks) - 1)
            p, e, n = accmap.process_catalog(ch, cfg["seq_type"], cfg["categories"], cfg["statuses"], known)
            longest = max((len(x) for x in lines_of(ch)), default=0)
            assert rep == dict(lines=n, passing=p, put=len(e), refused=0, first_bad_line=-1, longest_line=longest), (i, rep, p, len(e), n)
            entries += e
            passing += p
        s, dup, conflicts = accmap.finish(entries)
        assert m.finish() == (len(entries), passing, dup, conflicts)
        slots, nodes, regions = m.fetch()
        assert ga.slot_accessions(slots) == [k for k, _ in s]
        assert nodes.tolist() == [n for _, n in s]
        assert regions.tolist() == np.bincount([n for _, n in entries], minlength=len(known)).tolist()
        return m, s
    except BaseException:
        m.close()
        raise


def first_bad_line(text, cfg):
    for i, ln in enumerate(lines_of(text)):
        if not accmap.in_grammar(ln, cfg["seq_type"], cfg["categories"], cfg["statuses"]):
            return i
    return -1


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked_cases(name):
    """inside the grammar: the hand-worked values; outside: refused at the first bad line (the host parser's then)"""
    text, over, passing, entries, n_lines, throws = CASES[name]
    cfg = cfg_of(name)
    bad = first_bad_line(text, cfg)
    if bad < 0:
        assert throws is None
        m, s = check([text], **over)
        assert m.n_passing == passing and sorted(s) == sorted(entries)
        m.close()
        return
    m, _ = new_map(**over)
    rep = m.submit(text, last=True)
    assert rep["refused"] == 1 and rep["first_bad_line"] == bad and rep["passing"] == 0 and rep["put"] == 0, rep
    assert m.finish() == (0, 0, 0, 0)
    m.close()


def sized_chunk(total, pad, seed):
    """`total` bytes of generated lines behind a pad line of pad + 6 bytes, the last line a filler"""
    head = filler(pad + 6)
    body = b""
    for ln in lines_of(catalog(total // 40 + 2, seed=seed)):
        if len(head) + len(body) + len(ln) + 40 > total:
            break
        body += ln
    return head + body + filler(total - len(head) - len(body))


@pytest.mark.parametrize("total", [TILE - 1, TILE, TILE + 1, 3 * TILE + 100, 40 * TILE + 7])
def test_scan_at_sizes_where_it_changes_shape(total):
    """a line start on every offset relative to a 16-byte lane border: the pad line in front grows byte by byte"""
    chunks = [sized_chunk(total, pad, seed=total + pad) for pad in range(17)]
    assert all(len(c) == total for c in chunks)
    check(chunks)[0].close()


def test_one_line_chunks_and_an_unterminated_tail():
    chunks = [L("7", "NC_1"), L("11", "NC_2"), L("562", "WP_2"), b"\n", L("9606", "NZ_3", nl="")]
    check(chunks)[0].close()
    m, _ = new_map()
    assert m.submit(L("9606", "NZ_3", nl=""), last=False)["refused"] == 1  # not the end of the stream: no whole line
    m.close()


SLIDERS = [L("9606", "NC_%06d.1", cat="complete|bacteria", status="xREVIEWEDx", name="Homo sapiens"),
           # fields that reach beyond the 32 bytes behind a tile and the 16 in front of it
           L("10090", "NZ_%06d.1", cat="c" * 150 + "|other", status="s" * 90 + "na", name="n" * 120)]


@pytest.mark.parametrize("which", [0, 1])
def test_every_field_straddles_a_tile_border(which):
    """a passing line slides byte by byte across the border between two tiles (which is a lane border too): each of its tabs, its
    tax id, its prefix, its category match and its status match lie across the border in one of the chunks"""
    line = SLIDERS[which]
    chunks = []
    for shift in range(0, len(line) + 1, 1 if which == 0 else 3):
        mine = line.replace(b"%06d", b"%06d" % shift)
        chunks.append(filler(2 * TILE - shift) + mine + L("7", "NC_9") + filler(100))
    _, s = check(chunks)
    assert len(s) == 2 * len(chunks)


def test_scan_blocks_beyond_one_workgroup_of_block_sums():
    """more than 1024 tiles: the prefix over the per-tile sums runs a stretch of tiles per thread"""
    text = catalog(75000, seed=3)
    assert len(text) > 1025 * TILE
    m, s = check([text])
    assert len(s) > 5000
    m.close()


def test_finish_of_more_than_2_16_entries_and_its_ties():
    """about 70 000 entries: more than one sort tile; equal keys stay in input order (check() compares the nodes)"""
    rows = [L(KNOWN[i % 4], "NC_%06d.%d" % (i * 7919 % 10007, i % 3)) for i in range(70000)]
    m, s = check([b"".join(rows[:40000]), b"".join(rows[40000:])], reserve=1)
    assert len(s) == 70000 and m.n_duplicates > 1000 and m.n_conflicts > 1000
    m.close()


@pytest.mark.parametrize("n", [0, 1, 2])
def test_finish_of_few_entries(n):
    check([b"".join([L("562", "WP_1")] + [L("7", "NC_%d" % (2 - i)) for i in range(n)])])[0].close()


def test_finish_of_equal_keys():
    m, s = check([b"".join(L(KNOWN[(i * 5) % 3], "NC_000001.11") for i in range(300))])
    assert m.n_duplicates == 299 and m.n_conflicts == 299
    m.close()


def test_key_lengths_and_word_borders():
    """accessions of 3 .. 31 bytes from the device, of 0 and 1 through append; keys that differ in their last byte, in byte 8 of the
    slot (the border between its first two words) and in their length alone"""
    lens = [3, 7, 8, 9, 15, 16, 17, 30, 31]
    accs = ["NC_" + "A" * (n - 3) for n in lens] + ["NC_" + "A" * (n - 4) + "B" for n in lens if n > 3]
    accs += ["NC_0000" + c + "00" for c in "012"] + ["NC_0000" + c for c in "012"]  # slot byte 8 is key byte 7
    accs += ["WP_" + "A" * 29]  # 32 bytes in a line that does not pass: no refusal
    m, cfg = new_map()
    text = b"".join(L(KNOWN[i % 4], a) for i, a in enumerate(accs))
    rep = m.submit(text)
    p, entries, _ = accmap.process_catalog(text, cfg["seq_type"], cfg["categories"], cfg["statuses"], KNOWN)
    assert rep["refused"] == 0 and rep["put"] == len(entries) == len(accs) - 1
    extra = [(b"", 1), (b"N", 2), (b"O", 0), (b"", 3)]
    m.append([k for k, _ in extra], [n for _, n in extra])
    bad = L("7", "NC_" + "A" * 29)
    rep = m.submit(L("562", "NC_1") + bad)
    assert rep["refused"] == 1 and rep["first_bad_line"] == 1
    s, dup, conflicts = accmap.finish(entries + extra)
    assert m.finish() == (len(s), p + len(extra), dup, conflicts) and dup == 1
    slots, nodes, _ = m.fetch()
    assert ga.slot_accessions(slots) == [k for k, _ in s] and nodes.tolist() == [n for _, n in s]
    first = accmap.first_nodes(entries + extra)
    headers = [b"> x", b">N x", b">NC_" + b"A" * 28 + b" x", b">NC_" + b"A" * 29 + b" x", b">NC_00001 x", b">NC_000010 x", b">NC_0000100 x"]
    want = [accmap.lookup(first, h) for h in headers]
    assert want[:2] == [1, 2] and want[2] >= 0 and want[3] == -1 and want[4] >= 0 and want[5] == -1 and want[6] >= 0
    assert m.lookup(headers).tolist() == want
    m.close()


def test_growth_from_one_entry():
    chunks = [catalog(400, seed=s) for s in (21, 22, 23)]
    check(chunks, reserve=1)[0].close()


REFUSED = {
    "four_tabs": (L("7", "NC_1") + b"7\tx\tNC_9\tbacteria\tREVIEWED\n" + L("7", "NC_2"), 1),
    "no_tabs": (b"hello\n", 0),
    "nul": (L("7", "NC_1") * 3 + L("7", "WP_1", name="a\0b"), 3),
    "high_byte_in_a_passing_accession": (L("7", "NC_1") + L("7", "NC_1").replace(b"NC_1", b"NC_1\xc3\xa9"), 1),
    "line_of_2049": (_sized(2048) + _sized(2049) + _sized(2050), 1),
    "line_longer_than_a_tile": (L("7", "NC_1") + b"y" * 9000 + b"\t\t\t\t\t\n" + L("7", "NC_2"), 1),
    "tax_id_leading_zero": (L("7", "NC_1") + L("07", "NC_2"), 1),
    "tax_id_ten_digits": (L("1234567890", "NC_2"), 0),
    "tax_id_empty": (L("", "NC_2"), 0),
    "tax_id_non_digit": (L("7", "WP_1") * 100 + L("7 ", "NC_2"), 100),
    "accession_of_32": (L("7", "NC_" + "1" * 29), 0),
    "unterminated_in_mid_stream": (L("7", "NC_1") + L("7", "NC_2", nl=""), 1),
}


def test_a_refused_chunk_leaves_the_handle_as_it_was():
    m, cfg = new_map()
    good1, good2 = catalog(300, seed=31), catalog(300, seed=32)
    assert m.submit(good1)["refused"] == 0
    for name, (text, bad) in REFUSED.items():
        assert first_bad_line(text, cfg) == bad or name == "unterminated_in_mid_stream", name
        rep = m.submit(text)
        assert (rep["refused"], rep["first_bad_line"], rep["passing"], rep["put"]) == (1, bad, 0, 0), (name, rep)
    # a high byte in an accession that does not pass, a tax id that is no number on a line that does not pass: no refusal
    fine = L("x", "WP_\xe9") + L("007", "NC_1", status="MODEL")
    assert m.submit(fine)["refused"] == 0
    assert m.submit(good2)["refused"] == 0
    p, entries, _ = accmap.process_catalog(good1 + good2, cfg["seq_type"], cfg["categories"], cfg["statuses"], KNOWN)
    s, dup, conflicts = accmap.finish(entries)
    assert m.finish() == (len(s), p, dup, conflicts)
    slots, nodes, regions = m.fetch()
    assert ga.slot_accessions(slots) == [k for k, _ in s] and nodes.tolist() == [n for _, n in s]
    assert regions.tolist() == np.bincount([n for _, n in entries], minlength=len(KNOWN)).tolist()
    m.close()


def test_append_between_device_chunks_keeps_input_order():
    m, _ = new_map()
    assert m.submit(L("7", "NC_5") + L("562", "NC_4"))["put"] == 2
    m.append([b"NC_5", b"NC_4"], [1, 3], n_passing=5)
    assert m.submit(L("9606", "NC_5"))["put"] == 1
    assert m.finish() == (5, 8, 3, 3)
    slots, nodes, regions = m.fetch()
    assert ga.slot_accessions(slots) == [b"NC_4"] * 2 + [b"NC_5"] * 3 and nodes.tolist() == [1, 3, 0, 1, 2]
    assert regions.tolist() == [1, 2, 1, 1]
    assert m.lookup([b">NC_5 x", b">NC_4 x"]).tolist() == [0, 1]
    m.close()


@pytest.fixture(scope="module")
def looked_up():
    text = catalog(3000, seed=41) + b"".join(L("7", p + "77.1") for p in ("AC_", "NC_", "NG_", "NT_", "NW_", "NZ_", "NM_", "XM_", "NR_", "XR_"))
    m, cfg = new_map(seq_type="ALL")
    assert m.submit(text)["refused"] == 0
    m.finish()
    _, entries, _ = accmap.process_catalog(text, "ALL", cfg["categories"], cfg["statuses"], KNOWN)
    yield m, accmap.finish(entries)[0], accmap.first_nodes(entries)
    m.close()


def test_lookup(looked_up):
    m, s, first = looked_up
    keys = [k for k, _ in s]
    conflicting = [a[0] for a, b in zip(s, s[1:]) if a[0] == b[0] and a[1] != b[1]]
    assert conflicting
    headers = [b">" + keys[0] + b" first", b">" + keys[-1] + b" last\n", b">" + conflicting[0] + b" twice", b">" + conflicting[-1] + b" twice",
               b">AA x", b">" + b"Z" * 31 + b" above", b">" + keys[len(keys) // 2][:-1] + b"! between", b">" + keys[0], b"> x", b" >x",
               b">" + b"N" * 32 + b" 32 bytes", b">" + keys[3] + b"\tno blank\n", b">", b""]
    for p in ("AC_", "NC_", "NG_", "NT_", "NW_", "NZ_", "NM_", "XM_", "NR_", "XR_", "WP_"):
        headers.append(b">" + p.encode() + b"77.1 Some genome, complete\r\n")
    for complete_only in (False, True):
        want = [accmap.lookup(first, h, complete_only) for h in headers]
        got = m.lookup(headers, complete_only=complete_only)
        assert got.tolist() == want, complete_only
        if not complete_only:
            assert want[0] == s[0][1] and want[1] >= 0 and want[4:14] == [-1] * 10 and want[14:] == [0] * 10 + [-1]
        else:
            assert want[14:] == [0, 0, -1, -1, -1, 0, 0, 0, 0, 0, -1]


def test_lookup_in_device_memory_and_from_a_genomes_handle(looked_up):
    import torch
    m, s, first = looked_up
    keys = [k for k, _ in s]
    rnd = np.random.RandomState(5)
    headers = []
    for i in range(5000):
        k = keys[rnd.randint(len(keys))] if i % 3 else b"NC_%06d.1" % rnd.randint(10 ** 6)
        headers.append(b">" + k + (b" Escherichia coli chromosome" if i % 11 else b""))
    headers[17] = b">"
    want = {c: [accmap.lookup(first, h, c) for h in headers] for c in (False, True)}
    off = np.concatenate([[0], np.cumsum([len(h) for h in headers])]).astype(np.uint64)
    flat = np.frombuffer(b"".join(headers), dtype=np.uint8)
    fasta = b"".join(h + b"\nACGT\n" for h in headers)
    g = ga.DeviceGenomes(0)
    assert g.scan(fasta)[0] == len(headers)
    for c in (False, True):
        assert m.lookup(headers, complete_only=c).tolist() == want[c]
        assert m.lookup(flat, off, complete_only=c).tolist() == want[c]
        d = m.lookup(torch.from_numpy(flat.copy()).cuda(), torch.from_numpy(off.view(np.int64).copy()).cuda(), complete_only=c)
        assert d.is_cuda and d.cpu().tolist() == want[c]
        assert m.lookup_genomes(g, complete_only=c).tolist() == want[c]
    assert sum(w >= 0 for w in want[False]) > sum(w >= 0 for w in want[True]) > 100
    # the genomes handle goes on as before
    hdr, hoff = g.headers()
    assert bytes(hdr) == b"".join(headers) and hoff.tolist() == off.tolist()
    g.close()


def test_state_and_argument_errors():
    m, _ = new_map()
    for call in (m.fetch, lambda: m.lookup([b">x y"]), lambda: m.lookup_genomes(ga.DeviceGenomes(0))):
        with pytest.raises(ga.GsError) as e:
            call()
        assert e.value.code == -5
    for call in (lambda: m.append([b"NC_1"], [4]), lambda: m.append([b"NC_1"], [-1]), lambda: m.append([b"NC_1"], [0], n_passing=0),
                 lambda: m.append(np.full((1, 32), 40, dtype=np.uint8), [0]), lambda: m.append(ga.accession_slots([b"\xe9"]), [0])):
        with pytest.raises(ga.GsError) as e:
            call()
        assert e.value.code == -1
    assert m.submit(b"")["lines"] == 0
    assert m.finish() == (0, 0, 0, 0)
    for call in (lambda: m.submit(L("7", "NC_1")), lambda: m.append([b"NC_1"], [0]), m.finish):
        with pytest.raises(ga.GsError) as e:
            call()
        assert e.value.code == -5
    g = ga.DeviceGenomes(0)
    with pytest.raises(ga.GsError) as e:
        m.lookup_genomes(g)  # nothing scanned
    assert e.value.code == -5
    g.close()
    assert m.lookup([b">NC_1 x"]).tolist() == [-1] and m.lookup([]).tolist() == []
    assert m.fetch()[0].shape == (0, 32)
    m.close()
    with pytest.raises(ga.GsError) as e:
        ga.DeviceAccessionMap([7, 7], ["a"], ["b"])
    assert e.value.code == -1
    no_tree = ga.DeviceAccessionMap([], ["bacteria"], ["REVIEWED"])
    rep = no_tree.submit(L("7", "NC_1") * 3)
    assert (rep["passing"], rep["put"]) == (3, 0) and no_tree.finish() == (0, 3, 0, 0)
    no_tree.close()


def test_kernel_time():
    m, _ = new_map()
    assert m.kernel_time(True) == (0, 0.0)
    m.submit(catalog(500, seed=51))
    m.finish()
    m.lookup([b">NC_1 x"])
    n, ms = m.kernel_time(False)
    assert n == 4 and ms > 0  # count pass, write pass, finish, lookup
    m.close()
