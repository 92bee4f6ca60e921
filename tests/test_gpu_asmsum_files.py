"""gs_host_asmsum_files on the device against its own GS_HOST_FAST=0 result and against tests/asmsum.py: plain, gzip and BGZF files
cut into several chunks, a file with one CR LF line in the middle (one refused chunk), and the example's demo."""
import gzip
import os
import subprocess
import sys

import pytest

import asmsum
from conftest import ROOT, bgzf
from genestrip_amd import host

pytestmark = pytest.mark.gpu


def _as_tuples(picks):
    return [(node, e["taxid"], e["species_taxid"], e["ftp_url"], asmsum.QUALITIES.index(e["quality"]), e["is_reference"], e["line"])
            for node in sorted(picks) for e in picks[node]]


@pytest.fixture(scope="module")
def generated():
    known = sorted({7, 562, 9606, 10090} | {1000 + 13 * i for i in range(40)})
    return known, asmsum.summary(3000, known, seed=41)  # about 1 MB


@pytest.mark.parametrize("container", ["plain", "gz", "bgzf"])
def test_file_loop_against_the_host_path_and_the_restatement(container, generated, tmp_path, monkeypatch):
    known, text = generated
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", str(200000))  # several chunks, lines across reader blocks
    pack = {"plain": lambda d: d, "gz": gzip.compress, "bgzf": lambda d: bgzf(d, block=30000)}[container]
    tail = text[:text.rfind(b"\n", 0, 2000)]  # ... and an unterminated last line
    path = tmp_path / f"summary.txt{'' if container == 'plain' else '.gz'}"
    path.write_bytes(pack(text + tail))
    c = asmsum.cfg(known)
    entries, counted, short, skipped = asmsum.relevant_entries(text + tail, c)
    want = asmsum.cap(entries, 1)
    picks, total, totals = host.assembly_summary_files([path], known)
    assert _as_tuples(picks) == want and total == counted
    assert totals["lines"] == counted + short + skipped and totals["kept"] == len(entries) and totals["picked"] == len(want)
    assert totals["device_chunks"] >= 4 and totals["host_chunks"] == 1  # (the tail)
    assert len(entries) > 40 and len(entries) - len(want) > 10
    monkeypatch.setenv("GS_HOST_FAST", "0")
    picks_host, total_host, totals_host = host.assembly_summary_files([path], known)
    assert (picks_host, total_host) == (picks, total) and totals_host["device_chunks"] == 0
    for node in picks:
        for e in picks[node]:
            assert e["file_name"] == asmsum.file_name_of(e["ftp_url"])


def test_one_cr_lf_line_in_the_middle_gives_one_refused_chunk(generated, tmp_path, monkeypatch):
    known, text = generated
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", str(200000))
    at = text.find(b"\n", len(text) // 2)
    odd = text[:at] + b"\r" + text[at:]
    path = tmp_path / "summary.txt"
    path.write_bytes(odd)
    for kw in ({}, {"quality_mask": -1, "use_species_taxid": True}):
        c = asmsum.cfg(known, **kw)
        entries, counted, _, _ = asmsum.relevant_entries(odd, c)
        q = None if c["quality_mask"] == -1 else ("COMPLETE_LATEST", "CHROMOSOME_LATEST")
        picks, total, totals = host.assembly_summary_files([path], known, qualities=q, use_species_taxid=c["use_species_taxid"], max_per_taxid=2)
        assert _as_tuples(picks) == asmsum.cap(entries, 2) and total == counted
        assert totals["host_chunks"] == 1 and totals["device_chunks"] >= 3


def test_empty_ftp_names_file_and_line(generated, tmp_path):
    import genestrip_amd as ga
    from asmsum_cases import rec
    known, text = generated
    head = text[:text.rfind(b"\n", 0, 50000) + 1]
    path = tmp_path / "summary.txt"
    path.write_bytes(head + rec(ftp=b"") + b"\n" + head)
    with pytest.raises(ga.GsError) as e:
        host.assembly_summary_files([path], known)
    assert e.value.code == -1 and f"summary.txt: line {head.count(10) + 1}:" in str(e.value)


def test_example_demo():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "genbank_fastas.py"), "--demo"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "classified as 208962 Escherichia albertii" in r.stdout and "3 picked for 3 nodes" in r.stdout
