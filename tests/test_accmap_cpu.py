"""The accession map goals without a GPU: the plain-Python restatement (tests/accmap.py) against the hand-worked cases, its
grammar predicate, the slot encoding of the binding, and what the C ABI refuses before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import accmap
import genestrip_amd as ga
from accmap_cases import CASES, CFG, KNOWN, L, _sized, catalog, cfg_of


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_hand_worked_values(name):
    text, _, passing, entries, lines, throws = CASES[name]
    cfg = cfg_of(name)
    if throws is not None:
        with pytest.raises(accmap.Throws) as e:
            accmap.process_catalog(text, cfg["seq_type"], cfg["categories"], cfg["statuses"], KNOWN)
        assert e.value.line == throws
        return
    assert accmap.process_catalog(text, cfg["seq_type"], cfg["categories"], cfg["statuses"], KNOWN) == (passing, entries, lines)


def test_finish_orders_by_length_then_bytes_and_keeps_input_order_among_equals():
    _, entries, _ = accmap.process_catalog(CASES["duplicates"][0], "GENOMIC", CFG["categories"], CFG["statuses"], KNOWN)
    s, dup, conflicts = accmap.finish(entries + [(b"NC_", 3), (b"AC_9", 3), (b"NC_10", 0)])
    assert s == [(b"NC_", 3), (b"AC_9", 3), (b"NC_1", 0), (b"NC_1", 0), (b"NC_2", 1), (b"NC_2", 2), (b"NC_2", 1), (b"NC_10", 0)]
    assert (dup, conflicts) == (3, 2)
    first = accmap.first_nodes(entries)
    assert accmap.lookup(first, b">NC_2 Escherichia coli") == 1  # the first of the input, not the 9606 entry
    assert accmap.lookup(first, b">NC_2") == -1 and accmap.lookup(first, b"> NC_2 x") == -1 and accmap.lookup(first, b">NC_3 x") == -1
    assert accmap.lookup(first, b">NC_2 x", complete_only=True) == 1
    assert accmap.lookup(accmap.first_nodes([(b"NG_1", 2), (b"", 3)]), b">NG_1 x", complete_only=True) == -1
    assert accmap.lookup(accmap.first_nodes([(b"NG_1", 2), (b"", 3)]), b"> x") == 3


def test_grammar_predicate():
    g = lambda line: accmap.in_grammar(line, "GENOMIC", CFG["categories"], CFG["statuses"])
    assert g(L("7", "NC_1")) and g(b"\n") and g(L("7a", "WP_1")) and g(L("7", "NC_1", nl=""))
    assert g(L("7", "NC_" + "1" * 28)) and not g(L("7", "NC_" + "1" * 29)) and g(L("7", "WP_" + "1" * 40))
    assert not g(L("007", "NC_1")) and not g(L("0", "NC_1")) and not g(L("1234567890", "NC_1")) and not g(L("", "NC_1")) and not g(L("7a", "NC_1"))
    assert not g(b"7\tx\tNC_1\tbacteria\tREVIEWED\n") and not g(L("7", "NC_1", name="a\0b")) and not g(L("7", "NC_1").replace(b"NC_1", b"NC_\xe9"))
    assert g(_sized(2048)) and not g(_sized(2049)) and g(_sized(2048)[:-1]) and not g(_sized(2049)[:-1])
    for line in catalog(300, seed=5).splitlines(keepends=True):
        assert g(line)


def test_generated_catalog_has_every_kind_of_line():
    text = catalog(3000, seed=1)
    passing, entries, lines = accmap.process_catalog(text, "GENOMIC", CFG["categories"], CFG["statuses"], KNOWN)
    s, dup, conflicts = accmap.finish(entries)
    assert lines == 3000 and 0 < len(entries) < passing < lines and dup > conflicts > 0


def test_slot_encoding():
    slots = ga.accession_slots([b"", b"NC_1", b"N" * 31])
    assert slots.shape == (3, 32) and slots[1].tolist() == [4, 78, 67, 95, 49] + [0] * 27 and slots[2, 0] == 31
    assert ga.slot_accessions(slots) == [b"", b"NC_1", b"N" * 31]
    with pytest.raises(ValueError):
        ga.accession_slots([b"N" * 32])
    # read as four big-endian words the slots order as the reference orders keys
    keys = [b"NC_10", b"NC_2", b"", b"NC_000001.11", b"NC_000001.10", b"AC_1", b"NC_00000", b"NC_00001", b"NC_0000A"]
    words = [tuple(int.from_bytes(bytes(s[8 * w:8 * w + 8]), "big") for w in range(4)) for s in ga.accession_slots(keys)]
    assert [k for _, k in sorted(zip(words, keys))] == sorted(keys, key=accmap.key_order)


def _cfg(n_cat=1, n_stat=1, cats=None, stats=None, known=(7,), reserve=0):
    from genestrip_amd.binding import _AccmapCfg
    cats = cats if cats is not None else [b"bacteria"] * max(n_cat, 0)
    stats = stats if stats is not None else [b"na"] * max(n_stat, 0)
    known = np.asarray(known, dtype=np.int32)
    cfg = _AccmapCfg(1, 0, 0, n_cat, n_stat, len(known), (C.c_char_p * max(len(cats), 1))(*cats), (C.c_char_p * max(len(stats), 1))(*stats),
                     known.ctypes.data_as(C.c_void_p), reserve)
    cfg._keep = known
    return cfg


def test_arguments_are_refused_before_any_device_call():
    """(there is no device on this machine: a call that reached one would answer -6)"""
    L_ = ga.lib()
    h = C.c_void_p()
    bad = [_cfg(n_cat=0), _cfg(n_cat=17, cats=[b"x"] * 17), _cfg(n_stat=0), _cfg(cats=[b""]), _cfg(stats=[b"x" * 33]), _cfg(known=(7, 7)),
           _cfg(known=(9, 7)), _cfg(known=(0, 7)), _cfg(reserve=-1)]
    for cfg in bad:
        assert L_.gs_accmap_create(C.byref(h), 0, C.byref(cfg)) == -1 and not h.value
    assert L_.gs_accmap_create(None, 0, C.byref(_cfg())) == -1
    assert L_.gs_accmap_create(C.byref(h), 0, None) == -1
    r = (C.c_int64 * 8)()
    assert L_.gs_accmap_submit(None, b"x", 1, 0, 0, r) == -1
    assert L_.gs_accmap_append(None, None, None, 0, 0) == -1
    assert L_.gs_accmap_finish(None, r) == -1
    assert L_.gs_accmap_fetch(None, None, None, None) == -1
    assert L_.gs_accmap_lookup(None, None, None, 0, 0, 0, None) == -1
    assert L_.gs_accmap_lookup_genomes(None, None, 0, None) == -1
    assert L_.gs_accmap_get_device(None, None) == -1 and L_.gs_accmap_kernel_time(None, 0, None, None) == -1
    assert L_.gs_accmap_destroy(None) == 0


@pytest.mark.skipif(ga.device_count() > 0, reason="only meaningful without a GPU")
def test_fails_loudly_without_gpu():
    with pytest.raises(ga.GsError) as e:
        ga.DeviceAccessionMap(KNOWN, CFG["categories"], CFG["statuses"])
    assert e.value.code == -6


# ---- the host layer without a device (GS_HOST_FAST=0): gs_host_accmap_files through gs_accmapparse.h into a host-only map
import gzip  # noqa: E402

from conftest import bgzf  # noqa: E402
from genestrip_amd import host  # noqa: E402


def _expect(streams, cfg):
    """the restatement over files that are streams of their own, into one map -> (passing, sorted entries, dup, conflicts, regions, lines)"""
    passing, entries, lines = 0, [], 0
    for data in streams:
        p, e, n = accmap.process_catalog(data, cfg["seq_type"], cfg["categories"], cfg["statuses"], KNOWN)
        passing, entries, lines = passing + p, entries + e, lines + n
    s, dup, conflicts = accmap.finish(entries)
    return passing, s, dup, conflicts, np.bincount([n for _, n in entries], minlength=len(KNOWN)).tolist(), lines


def _same_map(m, tot, want):
    passing, s, dup, conflicts, regions, lines = want
    slots, nodes, reg = m.fetch()
    assert (tot["lines"], tot["passing"], tot["put"]) == (lines, passing, len(s)) and (m.n_entries, m.n_passing) == (len(s), passing)
    assert ga.slot_accessions(slots) == [k for k, _ in s] and nodes.tolist() == [n for _, n in s] and reg.tolist() == regions


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_layer_on_the_hand_worked_cases(name, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    text, _, passing, entries, lines, throws = CASES[name]
    cfg = cfg_of(name)
    path = tmp_path / "c.catalog"
    path.write_bytes(text)
    if throws is not None:
        with pytest.raises(ga.GsError) as e:
            host.accmap_files([path], KNOWN, **cfg)
        assert e.value.code == -1 and str(path) in str(e.value) and f"line {throws}:" in str(e.value)
        return
    m, tot = host.accmap_files([path], KNOWN, **cfg)
    assert m.device == -1 and tot["device_chunks"] == 0 and tot["host_chunks"] == 1
    _same_map(m, tot, _expect([text], cfg))
    assert sorted(ga.slot_accessions(m.fetch()[0])) == sorted(k for k, _ in entries) and tot["passing"] == passing and tot["lines"] == lines
    first = accmap.first_nodes(entries)
    headers = [b">" + k + b" x" for k, _ in entries] + [b">NC_404 x", b">NC_1"]
    for c in (False, True):
        assert m.lookup(headers, complete_only=c).tolist() == [accmap.lookup(first, h, c) for h in headers]
    m.close()
    none, tot2 = host.accmap_files([path], KNOWN, count_only=True, **cfg)
    assert none is None and (tot2["passing"], tot2["lines"]) == (passing, lines)


@pytest.mark.parametrize("container", ["plain", "gz", "bgzf"])
def test_host_layer_on_generated_files(container, tmp_path, monkeypatch):
    """two files into one map; the second ends without a newline and has the oddities of the hand-worked cases between its lines"""
    monkeypatch.setenv("GS_HOST_FAST", "0")
    pack = {"plain": lambda d: d, "gz": gzip.compress, "bgzf": lambda d: bgzf(d, block=4000)}[container]
    a = catalog(4000, seed=61)
    odd = [CASES[n][0] for n in ("two_tabs_pass_by_overlap", "four_tabs", "nul_bytes", "one_tab_and_none")]
    b = b"".join(ln + (odd[i % 4].rstrip(b"\0") if i % 97 == 0 else b"") for i, ln in enumerate(catalog(3000, seed=62).splitlines(keepends=True)))[:-1]
    paths = [tmp_path / ("a.catalog" + ("" if container == "plain" else ".gz")), tmp_path / ("b.catalog" + ("" if container == "plain" else ".gz"))]
    for p, d in zip(paths, (a, b)):
        p.write_bytes(pack(d))
    want = _expect([a, b], CFG)
    assert want[2] > want[3] > 0
    m, tot = host.accmap_files(paths, KNOWN, **CFG)
    _same_map(m, tot, want)
    m.close()
    assert host.accmap_files(paths, KNOWN, count_only=True, **CFG)[1]["passing"] == want[0]


def test_host_layer_errors_name_file_and_line(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    good = catalog(500, seed=63)
    long_key, long_line = tmp_path / "k.catalog", tmp_path / "l.catalog.gz"
    long_key.write_bytes(good + L("7", "NC_" + "1" * 29))
    long_line.write_bytes(gzip.compress(good + _sized(2049) + good))
    with pytest.raises(ga.GsError) as e:
        host.accmap_files([long_key], KNOWN, **CFG)
    assert e.value.code == -4 and str(long_key) in str(e.value) and "NC_" + "1" * 29 in str(e.value)
    assert host.accmap_files([long_key], KNOWN, count_only=True, **CFG)[1]["passing"] > 0  # (nothing is put: nothing to refuse)
    with pytest.raises(ga.GsError) as e:
        host.accmap_files([tmp_path / "k.catalog", long_line], KNOWN, count_only=True, **CFG)
    assert e.value.code == -1 and str(long_line) in str(e.value) and "line 501:" in str(e.value)
    with pytest.raises(ga.GsError) as e:
        host.accmap_files([tmp_path / "missing.catalog"], KNOWN, **CFG)
    assert e.value.code == -7
    with pytest.raises(ga.GsError) as e:
        host.accmap_files([long_key], [7, 7], **CFG)
    assert e.value.code == -1


def test_host_only_map_and_mapped_genome_files(tmp_path, monkeypatch):
    """no device anywhere: a host-only map answers the header lines of FASTA files (LF, CRLF, a header without a blank, a NUL byte)
    inside gs_host_genome_files_mapped as the restatement does"""
    monkeypatch.setenv("GS_HOST_FAST", "0")
    m = ga.DeviceAccessionMap(KNOWN, CFG["categories"], CFG["statuses"], device=-1)
    entries = [(b"NC_2", 1), (b"NC_1", 0), (b"NG_7", 3), (b"NC_2", 2), (b"", 3)]
    m.append([k for k, _ in entries], [n for _, n in entries])
    with pytest.raises(ga.GsError) as e:
        m.submit(L("7", "NC_1"))
    assert e.value.code == -4
    assert m.finish() == (5, 5, 1, 1) and m.kernel_time() == (0, 0.0)
    first = accmap.first_nodes(entries)
    headers = [b">NC_2 two", b">NG_7 x", b">NC_1", b">NC_9 x", b"> x", b">NC_1 \0x"]
    fa = tmp_path / "a.fa"
    fa.write_bytes(b"".join(h + (b"\r\n" if i % 2 else b"\n") + b"ACGTACGTAC\nGGG\n" for i, h in enumerate(headers)))
    for complete in (False, True):
        seen, regions = [], []

        def resolve(file, first_record, nodes):
            seen.extend(nodes.tolist())
            return nodes

        t = host.genome_files_mapped([fa], m, resolve, lambda seq, off, vi: regions.append((bytes(seq), off.tolist(), vi.tolist())), complete_only=complete)
        want = [accmap.lookup(first, h, complete) for h in headers]
        assert seen == want and t.records == len(headers) and t.kept_records == sum(w >= 0 for w in want)
        assert [v for _, _, vi in regions for v in vi] == [w for w in want if w >= 0]
        assert all(seq == b"ACGTACGTACGGG" * (len(off) - 1) for seq, off, _ in regions)
    m.close()
