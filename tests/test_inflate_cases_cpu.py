"""The catalogue of DEFLATE streams zlib never writes (tests/inflate_cases.py) against zlib itself, and the host decoders (GsInflate behind
host.gunzip, GsParallelGunzip behind host.gunzip_parallel) against the catalogue -- no GPU needed.  zlib is the reference throughout: a
legal case that zlib does not inflate to the intended text is a mistake of the writer, not a case."""
import os
import shutil
import subprocess
import zlib

import pytest

import deflatewriter as dw
import inflate_cases as ic
from genestrip_amd import host

LEGAL = {c.name: c for c in ic.legal()}
REJECTED = {c.name: c for c in ic.rejected()}


def test_the_writer_itself():
    """bit order, canonical codes and the two wrappers, on streams small enough to read"""
    d = dw.Deflate().stored(True, b"abc")
    assert d.payload() == b"\x01\x03\x00\xfc\xffabc"
    d = dw.Deflate().fixed(True, [97, 98, 99, (6, 3)])
    assert zlib.decompress(d.payload(), -15) == b"abcabcabc" == dw.apply([97, 98, 99, (6, 3)])
    assert [n for _, n, _ in d.records] == [8, 8, 8, 7 + 5]
    assert dw.canonical([2, 1, 3, 3]) == [0b01, 0b0, 0b011, 0b111]  # RFC 1951 3.2.2: B 0, A 10, C 110, D 111 -- low bit first
    assert dw.length_symbol(258) == (28, 0) and dw.length_symbol(258, True) == (27, 31) and dw.length_symbol(257) == (27, 30)
    assert dw.dist_symbol(32768) == (29, 8191) and dw.dist_symbol(1) == (0, 0) and dw.dist_symbol(24577) == (29, 0)
    assert sorted(dw.chain_code(list(range(16))).values()) == list(range(1, 15)) + [15, 15]
    import random
    for skew in (0.0, 0.5, 0.98):
        code = dw.random_complete_code(random.Random(1), list(range(286)), 15, skew)
        assert len(code) == 286 and dw.kraft(code.values()) == 32768 and max(code.values()) <= 15
    assert dw.cl_runs([0] * 140 + [5] * 8 + [0, 0]) == [(18, 127), (0, 0), (0, 0), (5, 0), (16, 3), (5, 0), (0, 0), (0, 0)]
    import gzip
    assert gzip.decompress(dw.gzip_member(d.payload(), b"abcabcabc")) == b"abcabcabc"
    assert gzip.decompress(dw.bgzf_member(d.payload(), b"abcabcabc")) == b"abcabcabc"


@pytest.mark.parametrize("name", sorted(LEGAL))
def test_zlib_inflates_every_legal_case_to_its_text(name):
    assert zlib.decompress(LEGAL[name].payload, -15) == LEGAL[name].text


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_zlib_rejects_every_damaged_case(name):
    with pytest.raises(zlib.error):
        zlib.decompress(REJECTED[name].payload, -15)


def test_the_cases_cover_what_they_are_there_for():
    g = ic.groups()
    assert {"one_dist_code", "no_dist_code", "deep48", "random_codes", "dense", "first_group_sizes", "alt258", "tiny_blocks", "stored_extremes",
            "header_extremes", "nested_gzip"} == set(g)
    for c in g["deep48"]:  # 48-bit tokens at every bit offset mod 32, at least four across a 256-byte boundary of the payload
        assert c.cover["offsets"] == list(range(32)) and c.cover["straddle"] >= 4 and c.cover["deep"] >= 200, c.cover
    assert len(g["random_codes"]) == 40 and sum(c.cover["blocks"] for c in g["random_codes"]) >= 100
    mass = {c.name: c.cover["mass"] for c in g["dense"]}
    assert mass == dict(dense_one_1bit=4, dense_two_2bit=4, dense_four_3bit=4, dense_three_3bit=3, dense_well_above=7, dense_eob_every_lane=4)
    for c in g["first_group_sizes"][:2]:
        assert c.cover["totals"] == list(range(250, 263))
    assert {(t, m) for t, m, _ in g["first_group_sizes"][2].cover["shorts"]} == {(t, m) for t in (257, 280) for m in (15, 16, 17, 18)}
    assert g["alt258"][0].cover["alt"] >= 50 and g["alt258"][0].cover["plain"] >= 20
    t = g["tiny_blocks"][0].cover
    assert t["blocks"] >= 600 and min(t["kinds"].values()) >= 150 and min(t["empty"].values()) >= 10 and t["pads"] == list(range(8))
    assert t["into_stored"] >= 20 and t["across"] >= 100
    h = {c.name: c for c in g["header_extremes"]}
    assert h["header_run16_across_the_seam"].cover["seam"] and h["header_all_18_runs"].cover["full18"] >= 1
    assert len(REJECTED) == 15


@pytest.mark.parametrize("group", sorted(ic.groups()))
def test_host_decoders_on_legal_cases(group):
    for c in ic.groups()[group]:
        z = dw.gzip_member(c.payload, c.text)
        for block in (1 << 20, 5000, 333) if len(c.text) < 200_000 else (1 << 20, 5000):
            assert host.gunzip(z, len(c.text), block) == c.text, (c.name, block)
        for threads in (1, 3):
            for chunk in (4096, 65536):
                assert host.gunzip_parallel(z, len(c.text), threads, chunk, 77_777) == c.text, (c.name, threads, chunk)
        if not c.gzip_only:  # the same payload as a BGZF member: the block-parallel reader
            assert host.gunzip_parallel(dw.bgzf_member(c.payload, c.text), len(c.text), 3) == c.text, c.name


def test_host_decoders_reject_damaged_cases():
    for c in ic.rejected():
        z = dw.gzip_member(c.payload, c.text)
        with pytest.raises(RuntimeError):
            host.gunzip(z, len(c.text) + 65536, 5000)
        for threads, chunk in ((1, 4096), (3, 65536)):
            with pytest.raises(RuntimeError):
                host.gunzip_parallel(z, len(c.text) + 65536, threads, chunk)
        with pytest.raises(RuntimeError):
            host.gunzip_parallel(dw.bgzf_member(c.payload, c.text), len(c.text) + 65536, 3)


def test_catalogue_streams_under_sanitizers(tmp_path):
    """a handful of the streams through tests/native/gunzip_sanitize.cpp, the stand-alone harness of tests/test_host_cpu.py, built with
    AddressSanitizer and UndefinedBehaviorSanitizer: it reads them from files"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(os.path.dirname(__file__), "native", "gunzip_sanitize.cpp")
    exe = str(tmp_path / "gunzip_sanitize")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=alignment", "-std=c++17", "-pthread"]
    b = subprocess.run(["g++", *flags, "-o", exe, src, "-lz"], capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    args = []
    names = ["one_dist_code_sym0", "one_dist_code_sym29", "no_dist_code", "deep48_0", "random_codes_00", "random_codes_09", "dense_eob_every_lane",
             "first_group_sizes_far", "alt258", "tiny_blocks", "stored_extremes", "header_cl7_minimal", "header_run16_across_the_seam"]
    for name in names:
        c = LEGAL[name]
        (tmp_path / (name + ".gz")).write_bytes(dw.gzip_member(c.payload, c.text))
        (tmp_path / (name + ".txt")).write_bytes(c.text)
        args += [str(tmp_path / (name + ".gz")), str(tmp_path / (name + ".txt"))]
    for name in ("rejected_distance_beyond_the_start", "rejected_length_without_distance_code", "rejected_oversubscribed_literal_code",
                 "rejected_ends_inside_a_token", "rejected_run_past_the_lengths"):
        c = REJECTED[name]
        (tmp_path / (name + ".gz")).write_bytes(dw.gzip_member(c.payload, c.text))
        args += [str(tmp_path / (name + ".gz")), "-"]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fails 0" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
