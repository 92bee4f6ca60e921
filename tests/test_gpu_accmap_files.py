"""host.accmap_files (gs_host_accmap_files: RefSeq catalog files -> the accession map, chunks on the device, what it refuses through
gs_accmapparse.h) and host.genome_files_mapped (the genome file loop with the map in front of the resolver) against the
plain-Python restatement (tests/accmap.py) and against the same calls under GS_HOST_FAST=0.  Needs an MI355X: run with -m gpu."""
import gzip

import numpy as np
import pytest

import accmap
import genestrip_amd as ga
from accmap_cases import CFG, KNOWN, L, catalog
from conftest import bgzf
from genestrip_amd import host
from progresscheck import check_records, run

pytestmark = pytest.mark.gpu

SMALLEST_BLOCK = 64  # reader_shape() of gs_host.cpp takes GS_HOST_BLOCK_BYTES from 64 on
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _pack(container, data):
    return data if container == "plain" else gzip.compress(data, 6) if container == "gz" else bgzf(data, block=3000)


def _short_catalog(n, seed):
    """lines of 25 to 40 bytes, so that they fit reader blocks of 64 bytes and straddle them"""
    rng = np.random.default_rng(seed)
    tax = ["7", "562", "9606", "10090", "11"]
    pre = ["NC_", "NZ_", "WP_", "NG_", "XP_"]
    cat = ["bacteria", "other", "plant"]
    st = ["REVIEWED", "na", "MODEL"]
    return b"".join(L(tax[int(rng.integers(5))], pre[int(rng.integers(5))] + str(int(rng.integers(400))), cat=cat[int(rng.integers(3))],
                      status=st[int(rng.integers(3))], name="s" * int(rng.integers(1, 6)), tail=str(int(rng.integers(99)))) for _ in range(n))


def _expect(streams):
    passing, entries, lines = 0, [], 0
    for data in streams:
        p, e, n = accmap.process_catalog(data, CFG["seq_type"], CFG["categories"], CFG["statuses"], KNOWN)
        passing, entries, lines = passing + p, entries + e, lines + n
    s, dup, conflicts = accmap.finish(entries)
    return passing, s, np.bincount([n for _, n in entries], minlength=len(KNOWN)).tolist(), lines


def _map_of(m, tot):
    slots, nodes, regions = m.fetch()
    return tot["passing"], list(zip(ga.slot_accessions(slots), nodes.tolist())), regions.tolist(), tot["lines"]


ODD = [b"7\tx\tNC_9\tbacteria\tREVIEWED\n", b"7\tx\tN\0C_1\tbact\0eria\tREVIEWED\t1\n", b"bacteria\tREVIEWED\tNC_5\n", L("007", "NC_3"), b"\n"]


@pytest.mark.parametrize("container", ["plain", "gz", "bgzf"])
@pytest.mark.parametrize("block", [SMALLEST_BLOCK, 4096])
def test_files_into_one_map(container, block, tmp_path, monkeypatch):
    """two files, the second with lines outside the device's grammar between chunks that the device takes, and without a final
    newline: equal to the restatement and to the call under GS_HOST_FAST=0"""
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", str(block))
    make = _short_catalog if block == SMALLEST_BLOCK else catalog
    a = make(1500, 71)
    parts = [make(400, 72 + i) + ODD[i] for i in range(len(ODD))] + [make(400, 80)]
    b = b"".join(parts)[:-1]
    paths = []
    for name, data in (("a", a), ("b", b)):
        paths.append(tmp_path / (name + ".catalog" + ("" if container == "plain" else ".gz")))
        paths[-1].write_bytes(_pack(container, data))
    want = _expect([a, b])
    assert len(want[1]) > 100
    m, tot = host.accmap_files(paths, KNOWN, **CFG)
    got = _map_of(m, tot)
    assert got == want, (tot, got[0], want[0], len(got[1]), len(want[1]))
    assert tot["device_chunks"] > 0 and tot["host_chunks"] > 0 and m.device == 0
    first = accmap.first_nodes(want[1])
    headers = [b">" + k + b" x" for k, _ in want[1][::7]] + [b">NC_404 x"]
    assert m.lookup(headers, complete_only=True).tolist() == [accmap.lookup(first, h, True) for h in headers]
    m.close()
    none, tot2 = host.accmap_files(paths, KNOWN, count_only=True, **CFG)
    assert none is None and (tot2["passing"], tot2["lines"], tot2["device_chunks"] > 0) == (want[0], want[3], True)
    monkeypatch.setenv("GS_HOST_FAST", "0")
    mh, toth = host.accmap_files(paths, KNOWN, **CFG)
    assert _map_of(mh, toth) == want and toth["device_chunks"] == 0 and mh.device == -1
    mh.close()


def test_a_bad_file_fails_with_its_line(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "4096")
    good = catalog(600, 91)
    path = tmp_path / "bad.catalog"
    path.write_bytes(good + L("7", "NC_1", name="n" * 2100) + good)
    with pytest.raises(ga.GsError) as e:
        host.accmap_files([path], KNOWN, **CFG)
    assert e.value.code == -1 and str(path) in str(e.value) and "line 601:" in str(e.value)
    path.write_bytes(good + L("7", "NC_" + "1" * 29) + good)
    with pytest.raises(ga.GsError) as e:
        host.accmap_files([path], KNOWN, **CFG)
    assert e.value.code == -4 and "NC_" + "1" * 29 in str(e.value)


def test_progress_records_and_cancellation(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "4096")
    data = catalog(3000, 93)
    p = tmp_path / "c.catalog"
    p.write_bytes(data)
    paths = [str(p)]
    call = lambda: host.accmap_files(paths, KNOWN, **CFG)
    (m, tot), stop, records = run(call)
    assert stop is None and tot["lines"] == 3000 and tot["device_chunks"] > 10
    m.close()
    assert check_records(records, paths, complete=True)[0] == 3000
    got, stop, recs = run(call, stop_at=2)  # behind the first chunk
    k = check_records(recs, paths, complete=False)[0]
    assert got is None and stop.code == -8 and 0 < k < 3000
    assert stop.totals["lines"] == k and stop.totals["passing"] == accmap.process_catalog(b"".join(data.splitlines(keepends=True)[:k]), **CFG, known_taxids=KNOWN)[0]
    assert not hasattr(stop, "map")


def _fasta(entries):
    """records for some of the map's accessions and for others: LF and CRLF lines, a header without a blank, an unknown accession"""
    rng = np.random.default_rng(95)
    keys = sorted({k for k, _ in entries})[:60]
    recs, headers = [], []
    for i, k in enumerate(keys + [b"NC_404404.1", b"WP_1.1"]):
        eol = b"\r\n" if i % 3 == 1 else b"\n"
        h = b">" + k + (b"" if i % 10 == 7 else b" Some species, complete genome")
        body = ACGT[rng.integers(0, 4, int(rng.integers(200, 3000)))].tobytes()
        headers.append(h + (b"\r" if eol == b"\r\n" else b""))
        recs.append(h + eol + b"".join(body[j:j + 70] + eol for j in range(0, len(body), 70)))
    return recs, headers


def test_genome_files_mapped_into_a_store(tmp_path, monkeypatch):
    """the records of two FASTA files resolved through the map on the device, into gs_dbbuild_add: the store of genome_files with a
    dictionary as resolver.  The second file has a NUL byte: its chunk goes through the host parser and is looked up by the same rule"""
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    cat = tmp_path / "c.catalog.gz"
    cat.write_bytes(gzip.compress(catalog(4000, 97)))
    m, tot = host.accmap_files([cat], KNOWN, **CFG)
    slots, nodes, _ = m.fetch()
    entries = list(zip(ga.slot_accessions(slots), nodes.tolist()))
    first = accmap.first_nodes(entries)
    recs, _ = _fasta(entries)
    f1, f2 = tmp_path / "a.fna", tmp_path / "b.fna.gz"
    f1.write_bytes(b"".join(recs[0::2]))
    f2.write_bytes(gzip.compress(b"".join(recs[1::2]) + b">" + entries[0][0] + b" with a NUL\nACGT\0ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n"))
    parent = np.array([-1, 0, 0, 1], dtype=np.int32)

    def build(walk):
        b = ga.DeviceDbBuilder(31, len(KNOWN), parent)
        totals = [walk(lambda s, o, v: b.add(s, o, v, update=u)) for u in (False, True)]
        out = b.finish()
        b.close()
        return out, totals

    seen = []

    def by_nodes(_file, _first, node):
        seen.extend(node.tolist())
        return node

    for complete in (False, True):
        del seen[:]
        by_dict = lambda _file, _first, headers: [accmap.lookup(first, h, complete) for h in headers]
        got, t_m = build(lambda add: host.genome_files_mapped([f1, f2], m, by_nodes, add, complete_only=complete))
        want, t_d = build(lambda add: host.genome_files([f1, f2], by_dict, add))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and len(got[0]) > 10000
        assert (t_m[0].records, t_m[0].kept_records, t_m[0].kept_bases) == (t_d[0].records, t_d[0].kept_records, t_d[0].kept_bases)
        assert t_m[0].host_chunks >= 1 and t_m[0].chunks > t_m[0].host_chunks and 0 < t_m[0].kept_records < t_m[0].records
        assert len(seen) == 2 * t_m[0].records and min(seen) == -1
    m.close()
