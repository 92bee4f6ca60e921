"""The fastasgenbank goal without a device: tests/asmsum.py on the hand-worked cases of tests/asmsum_cases.py, the host-only handle
(device -1) through the binding, and gs_host_asmsum_files under GS_HOST_FAST=0 -- gs_asmsumparse.h over plain, gzip and BGZF files,
fed in pieces small enough that lines span them and that CR and LF fall into different feeds."""
import gzip

import pytest

import asmsum
import genestrip_amd as ga
import progresscheck
from asmsum_cases import CAP_CASES, CASES, FILE_NAMES, KNOWN, cfg_of, rec
from conftest import bgzf
from genestrip_amd import host


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_hand_worked_values(name):
    text, _, entries, counted, short, skipped, throws, device = CASES[name]
    c = cfg_of(name)
    if throws is not None:
        with pytest.raises(asmsum.EmptyFtp) as e:
            asmsum.relevant_entries(text, c)
        assert e.value.line == throws
    else:
        assert asmsum.relevant_entries(text, c) == (entries, counted, short, skipped)
    assert asmsum.in_grammar(text, c, last=True) == device


def test_file_names():
    for ftp, want in FILE_NAMES:
        assert asmsum.file_name_of(ftp) == want
        assert ga.file_name_of(ftp) == want
        assert ga.file_name_of(ftp.decode()) == want
    with pytest.raises(ga.GsError) as e:
        ga.file_name_of(b"")
    assert e.value.code == -1


def _entries_of(qualities, node=1):
    return [(node, b"562", b"562", b"ftp%d" % i, q, False, i) for i, q in enumerate(qualities)]


@pytest.mark.parametrize("case", range(len(CAP_CASES)))
def test_cap_cases(case):
    qualities, max_per_node, left = CAP_CASES[case]
    entries = _entries_of(qualities)
    want = [entries[i] for i in left]
    assert asmsum.cap(entries, max_per_node) == want
    # two more nodes around it, one entry and none: they come out in node order and stay as they are
    around = [(3, b"10090", b"1", b"x", 5, True, 100)] + entries + [(0, b"7", b"7", b"y/", 10, False, 101)]
    with ga.DeviceAssemblySummary(KNOWN, device=-1) as h:
        h.append(around[:2], n_counted=5, n_lines=7)
        h.append(around[2:])
        assert h.finish(max_per_node) == (len(around), len(want) + 2, 3, 5 + len(around) - 2)
        assert h.fetch() == [around[-1]] + want + [around[0]]


def test_host_only_handle_states_and_arguments():
    h = ga.DeviceAssemblySummary(KNOWN, device=-1)
    with pytest.raises(ga.GsError) as e:
        h.submit(b"x\n")
    assert e.value.code == -4  # GS_E_UNSUPPORTED
    with pytest.raises(ga.GsError) as e:
        h.fetch()
    assert "behind gs_asmsum_finish" in str(e.value)
    for bad in ([(4, b"1", b"1", b"f", 1, False, 0)], [(-1, b"1", b"1", b"f", 1, False, 0)], [(0, b"1", b"1", b"f", 0, False, 0)],
                [(0, b"1", b"1", b"f", 11, False, 0)], [(0, b"1", b"1", b"", 1, False, 0)], [(0, b"1", b"1", b"f", 1, False, -1)]):
        with pytest.raises(ga.GsError) as e:
            h.append(bad)
        assert e.value.code == -1, bad
    with pytest.raises(ga.GsError):
        h.append([], n_counted=-1)
    assert h.finish(1) == (0, 0, 0, 0)
    assert h.fetch() == []
    for call in (lambda: h.append([]), lambda: h.finish(1)):
        with pytest.raises(ga.GsError) as e:
            call()
        assert "gs_asmsum_finish" in str(e.value)
    h.close()
    h.close()
    for kw in ({"known_taxids": [5, 5]}, {"known_taxids": [0]}, {"known_taxids": [1234567890]}, {"known_taxids": [1], "qualities": [11]},
               {"known_taxids": [1], "reserve_entries": -1}):
        with pytest.raises(ga.GsError) as e:
            ga.DeviceAssemblySummary(device=-1, **kw)
        assert e.value.code == -1, kw
    assert ga.quality_mask(None) == -1 and ga.quality_mask([]) == 0 and ga.quality_mask(("COMPLETE_LATEST", "CHROMOSOME_LATEST")) == asmsum.DEFAULT_MASK


def _want(text, c, max_per_node):
    entries, counted, _, _ = asmsum.relevant_entries(text, c)
    return asmsum.cap(entries, max_per_node), counted, entries


def _as_tuples(picks):
    return [(node, e["taxid"], e["species_taxid"], e["ftp_url"], asmsum.QUALITIES.index(e["quality"]), e["is_reference"], e["line"])
            for node in sorted(picks) for e in picks[node]]


def _files_kw(c, max_per_node):
    q = None if c["quality_mask"] == -1 else [i for i in range(11) if c["quality_mask"] >> i & 1]
    return {"selected": c["filter"], "qualities": q, "reference_only": c["reference_only"], "use_species_taxid": c["use_species_taxid"],
            "max_per_taxid": max_per_node}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_layer_on_the_hand_worked_cases(name, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    text, _, entries, counted, short, skipped, throws, _ = CASES[name]
    c = cfg_of(name)
    for piece in (1 << 20, 1, 7):
        monkeypatch.setenv("GS_HOST_BLOCK_BYTES", str(piece))
        path = tmp_path / f"{name}.txt"
        path.write_bytes(text)
        if throws is not None:
            with pytest.raises(ga.GsError) as e:
                host.assembly_summary_files([path], KNOWN, **_files_kw(c, 0))
            assert e.value.code == -1 and f"{name}.txt: line {throws}:" in str(e.value)
            continue
        picks, total, totals = host.assembly_summary_files([path], KNOWN, **_files_kw(c, 0))
        assert _as_tuples(picks) == asmsum.cap(entries, 0) and total == counted
        assert totals["lines"] == counted + short + skipped and totals["kept"] == len(entries) and totals["device_chunks"] == 0
        for node in picks:
            for e in picks[node]:
                assert e["file_name"] == asmsum.file_name_of(e["ftp_url"])


def _generated(seed, n_lines=1500):
    known = sorted({7, 562, 9606, 10090} | {1000 + 13 * i for i in range(40)})
    text = asmsum.summary(n_lines, known, seed=seed)
    return known, text


@pytest.mark.parametrize("container", ["plain", "gz", "bgzf"])
def test_host_layer_on_generated_files(container, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "333")  # (lines have 300 bytes and more: every one spans feeds)
    pack = {"plain": lambda d: d, "gz": gzip.compress, "bgzf": lambda d: bgzf(d, block=4000)}[container]
    known, text = _generated(21)
    lines = text.split(b"\n")
    # every third terminator a CR LF, some lone CRs, a U+0131 key: all of it host logic
    odd = b"".join(ln + (b"\r\n" if i % 3 == 0 else b"\r" if i % 11 == 0 else b"\n") for i, ln in enumerate(lines[:-1]))
    odd += rec(taxid=b"\xc4\xb1000", level=b"Contig").replace(b"c0", b"x" * 700) + b"\r"
    for which, data in (("lf", text), ("odd", odd)):
        path = tmp_path / f"summary_{which}.txt{'' if container == 'plain' else '.gz'}"
        path.write_bytes(pack(data))
        for kw in ({}, {"quality_mask": -1, "use_species_taxid": True}, {"filter": set(range(0, len(known), 2)), "quality_mask": 0x7fe, "reference_only": True}):
            c = asmsum.cfg(known, **kw)
            for max_per_node in (1, 3):
                want, counted, entries = _want(data, c, max_per_node)
                picks, total, totals = host.assembly_summary_files([path], known, **_files_kw(c, max_per_node))
                assert _as_tuples(picks) == want and total == counted and totals["kept"] == len(entries) and totals["picked"] == len(want)
            if not kw:
                assert len(entries) > 40 and len(entries) - len(want) > 10  # dozens kept, several nodes cut


def test_several_files_are_streams_of_their_own(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    a, b = rec() + b"\r", b"\n" + rec(taxid=b"7") + b"\n"  # (the CR that ends file a and the LF that starts file b are two terminators)
    (tmp_path / "a.txt").write_bytes(a)
    (tmp_path / "b.txt").write_bytes(b)
    picks, total, totals = host.assembly_summary_files([tmp_path / "a.txt", tmp_path / "b.txt"], KNOWN)
    assert total == 2 and totals["lines"] == 3
    assert _as_tuples(picks) == [(0, b"7", b"562", rec.__defaults__[5], 1, False, 2), (1, b"562", b"562", rec.__defaults__[5], 1, False, 0)]


def test_selected_given_and_empty_opens_no_file(tmp_path):
    assert host.assembly_summary_files([tmp_path / "not_there.txt"], KNOWN, selected=[])[:2] == ({}, 0)
    with pytest.raises(ga.GsError):
        host.assembly_summary_files([tmp_path / "not_there.txt"], KNOWN, selected=[1], device=-1)


def test_progress_and_cancellation(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_FAST", "0")
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "20000")
    known, text = _generated(22, 600)
    paths = [tmp_path / "one.txt", tmp_path / "two.txt"]
    for p in paths:
        p.write_bytes(text)
    n_lines = len(asmsum.lines_of(text))
    got, cancelled, records = progresscheck.run(lambda: host.assembly_summary_files(paths, known))
    assert cancelled is None and got[1] == 2 * asmsum.relevant_entries(text, asmsum.cfg(known))[1]
    assert progresscheck.check_records(records, [str(p) for p in paths], complete=True) == {0: n_lines, 1: n_lines}
    assert len(records) > 10
    got, cancelled, records = progresscheck.run(lambda: host.assembly_summary_files(paths, known), stop_at=4)
    assert got is None and cancelled is not None and len(records) == 5  # (the record of the stop follows the answer)
    reads = progresscheck.check_records(records, [str(p) for p in paths], complete=False)
    assert 0 < reads[0] < n_lines and 1 not in reads
