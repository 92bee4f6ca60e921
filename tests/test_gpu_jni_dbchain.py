"""The natives of the database-construction chain below the JVM: java/jni/gsgpu_jni.c compiled against the stand-in jni.h with the
functional JNIEnv of tests/native/jni_stub (as tests/test_gpu_jni.py does) and each group -- taxtree, accmap with genomes, asmsum,
their file-level calls and hostGenomeFilesInto -- driven as a JVM would drive it: Strings, String[], direct ByteBuffers with their
capacities in elements, int[] and long[].  Everything fetched must equal the ctypes path over the same C ABI (DeviceTaxTree,
DeviceAccessionMap, DeviceGenomes, DeviceAssemblySummary, host.*).  The stand-in's FindClass does not keep the class name, so an
IllegalArgumentException is recognised by the message only throw_short of the shim writes.  Needs an MI355X: run with -m gpu."""
import os
import types

import numpy as np
import pytest

import asmsum
import assembly
import genestrip_amd as ga
import genome_into as gi
import taxtree_cases
from accmap_cases import catalog
from conftest import GOLDEN
from genestrip_amd import host
from jnishim import I, J, SHORT, Z, build

pytestmark = pytest.mark.gpu

KNOWN = np.array([1, 2, 3], dtype=np.int32)    # the nodes of tests/golden/taxtree
CATS, STATS = ["bacteria", "other"], ["REVIEWED", "na"]


@pytest.fixture(scope="module")
def jni(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("jni") / "libgsjni_dbchain.so"))


# ---- taxtree
def _jni_tree_arrays(S, h, n):
    out = {k: np.full(max(n, 1), -7, dtype=np.int32) for k in ("taxids", "parent", "depth", "position", "subtree", "rank")}
    S.call("taxtreeFetch", None, J(h), *[x for k in out for x in S.buf(out[k])])
    off = np.zeros(n + 1, dtype=np.int64)
    S.call("taxtreeFetchNames", None, J(h), *S.buf(off), None, J(0))
    raw = np.zeros(max(int(off[n]), 1), dtype=np.uint8)
    S.call("taxtreeFetchNames", None, J(h), *S.buf(off), *S.buf(raw))
    ends = [int(o) if o >= 0 else -1 - int(o) for o in off]
    names = [raw.tobytes()[ends[i]:ends[i + 1]] if off[i] >= 0 else None for i in range(n)]
    return {k: v[:n] for k, v in out.items()}, names


def _same_tree(S, h, t):
    got, names = _jni_tree_arrays(S, h, t.n_nodes)
    want = t.arrays()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert names == t.names()


def test_taxtree_natives(jni, tmp_path):
    S = jni
    nodes_path, names_path = os.path.join(GOLDEN, "taxtree", "nodes.dmp"), os.path.join(GOLDEN, "taxtree", "names.dmp")
    golden = (open(nodes_path, "rb").read(), open(names_path, "rb").read())
    dump = taxtree_cases.random_dump(300, 17)
    ids = sorted({int(line.split(b"\t")[0]) for line in dump.splitlines()})
    named = b"".join(taxtree_cases.N(i, "name of %d" % i, "scientific name" if i % 3 else "synonym") for i in ids[::2])
    for nodes, names in (golden, (dump, named)):
        t = ga.DeviceTaxTree()
        t.submit_nodes(nodes, last=True)
        info = t.finish()
        t.submit_names(names, last=True)
        h = S.call("taxtreeCreate", J, I(0))
        rep = S.longs(8)
        # in front of finish: the library's own refusal, not a write into a buffer of unknown size
        assert b"gsgpu error" in S.call("taxtreeFetch", None, J(h), *[x for _ in range(6) for x in S.buf(np.zeros(4, dtype=np.int32))], throws=True)
        half = nodes.rfind(b"\n", 0, len(nodes) // 2) + 1
        S.call("taxtreeSubmitNodes", None, J(h), *S.text(nodes[:half]), Z(0), rep)
        assert S.get(rep, 4)[3] == 0
        S.call("taxtreeAppendNodes", None, J(h), *S.text(nodes[half:]), Z(1), rep)
        jinfo = S.longs(8)
        S.call("taxtreeFinishNodes", None, J(h), jinfo)
        assert S.get(jinfo, 7) == [info[k] for k in ("nodes", "reached", "max_depth", "duplicates", "on_host", "cycle_nodes", "slots")]
        half = names.rfind(b"\n", 0, len(names) // 2) + 1
        S.call("taxtreeSubmitNames", None, J(h), *S.text(names[:half]), Z(0), rep)
        S.call("taxtreeAppendNames", None, J(h), *S.text(names[half:]), Z(1))
        _same_tree(S, h, t)
        n = t.n_nodes
        assert S.call("taxtreeGetDevice", I, J(h)) == 0
        # select, small, regions_below
        req, exc = [n // 3, 0][:1 if n < 10 else 2], [n - 1]
        want_sel = t.select(req, exc, cut_rank="species")
        sel = np.zeros(n, dtype=np.uint8)
        count = S.call("taxtreeSelect", J, J(h), S.ints(req), J(len(req)), S.ints(exc), J(1), I(ga.RANK_NAMES.index("species")), *S.buf(sel))
        assert np.array_equal(sel, want_sel) and count == int(want_sel.sum())
        regions = (np.arange(n, dtype=np.int32) * 7) % 5
        want_small = t.small_tree(regions)
        outs = [np.zeros(max(t.n_reached, 1), dtype=np.int32) for _ in range(4)]
        n_small = S.call("taxtreeSmall", I, J(h), *S.buf(regions), I(4), *[x for o in outs for x in S.buf(o)])
        assert n_small == len(want_small["node_of_vi"])
        for o, k in zip(outs, ("node_of_vi", "parent_vi", "depth", "position")):
            assert np.array_equal(o[:n_small], want_small[k]), k
        selected = np.flatnonzero(t.select([0])).astype(np.int32)
        want_below, want_incl = t.regions_below(regions, selected, 9)
        incl, below = np.zeros(n, dtype=np.int32), np.zeros(len(selected), dtype=np.int32)
        n_below = S.call("taxtreeRegionsBelow", J, J(h), *S.buf(regions), S.ints(selected), J(len(selected)), I(9), I(-1), *S.buf(incl), *S.buf(below))
        assert np.array_equal(incl, want_incl) and np.array_equal(below[:n_below], want_below)
        arr = want = t.arrays()
        ref_incl = assembly.regions_inclusive(arr["parent"], regions)
        assert np.array_equal(np.asarray(ref_incl)[arr["depth"] >= 0], incl[arr["depth"] >= 0])
        # a stated capacity that is too small
        short = np.zeros(n - 1, dtype=np.int32)
        assert SHORT in S.call("taxtreeFetch", None, J(h), *S.buf(short), *[x for _ in range(5) for x in S.buf(None)], throws=True)
        assert SHORT in S.call("taxtreeSelect", J, J(h), S.ints(req), J(len(req) + 1), None, J(0), I(-1), *S.buf(sel), throws=True)
        assert SHORT in S.call("taxtreeSubmitNodes", None, J(h), *S.buf(np.zeros(8, dtype=np.uint8)), J(9), Z(1), rep, throws=True)
        S.call("taxtreeDestroy", None, J(h))
        t.close()
    # the file-level call on the golden dump, and the tax id file
    t, report = host.taxtree_files(nodes_path, names_path)
    rep = S.longs(8)
    h = S.call("hostTaxtreeFiles", J, I(0), S.string(nodes_path), S.string(names_path), rep)
    assert S.get(rep, 8) == [report[k] for k in ("nodes_lines", "names_lines", "device_chunks", "host_chunks", "nodes", "reached", "duplicates", "on_host")]
    _same_tree(S, h, t)
    S.call("taxtreeDestroy", None, J(h))
    t.close()
    missing = str(tmp_path / "no_such_nodes.dmp")
    assert b"no_such_nodes.dmp" in S.call("hostTaxtreeFiles", J, I(0), S.string(missing), None, rep, throws=True)
    ids_path = tmp_path / "taxids.txt"
    ids_path.write_bytes(taxtree_cases.TAXIDS_TEXT)
    want_req, want_exc = host.read_taxids_file(ids_path)
    assert (want_req.tolist(), want_exc.tolist()) == tuple(taxtree_cases.TAXIDS_NUMBERS)
    for through_file in (False, True):
        req, exc, counts = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.int32), S.longs(2)
        if through_file:
            S.call("hostReadTaxidsFile", None, S.string(ids_path), *S.buf(req), *S.buf(exc), J(16), counts)
        else:
            S.call("taxtreeReadTaxids", None, *S.text(taxtree_cases.TAXIDS_TEXT), *S.buf(req), *S.buf(exc), J(16), counts)
        n_req, n_exc = S.get(counts, 2)
        assert (req[:n_req].tolist(), exc[:n_exc].tolist()) == tuple(taxtree_cases.TAXIDS_NUMBERS)
    assert SHORT in S.call("hostReadTaxidsFile", None, S.string(ids_path), *S.buf(req), *S.buf(exc), J(17), counts, throws=True)


# ---- accmap and genomes
def _jni_map(S, h, n_entries, n_nodes):
    slots, nodes, regions = np.zeros((max(n_entries, 1), 32), dtype=np.uint8), np.zeros(max(n_entries, 1), dtype=np.int32), np.zeros(n_nodes, dtype=np.int32)
    S.call("accmapFetch", None, J(h), *S.buf(slots), *S.buf(nodes), *S.buf(regions))
    return slots[:n_entries], nodes[:n_entries], regions


def test_accmap_and_genomes_natives(jni, tmp_path):
    S = jni
    text = catalog(400, 5, known=KNOWN.tolist())
    extra = [b"NC_777777.1", b"NZ_XY01.1"]
    m = ga.DeviceAccessionMap(KNOWN, CATS, STATS)
    r = m.submit(text, last=True)
    m.append(extra, [2, 0], n_passing=3)
    info = m.finish()
    want = m.fetch()
    assert r["refused"] == 0 and info[0] > 20
    h = S.call("accmapCreate", J, I(0), Z(1), Z(0), Z(0), S.strings(CATS), S.strings(STATS), *S.buf(KNOWN), I(3), J(0))
    assert b"gsgpu error" in S.call("accmapFetch", None, J(h), *S.buf(None), *S.buf(None), *S.buf(np.zeros(3, dtype=np.int32)), throws=True)
    rep = S.longs(8)
    S.call("accmapSubmit", None, J(h), *S.text(text), Z(1), rep)
    assert S.get(rep, 6) == [r[k] for k in ("lines", "passing", "put", "refused", "first_bad_line", "longest_line")]
    S.call("accmapAppend", None, J(h), *S.buf(ga.accession_slots(extra)), *S.buf(np.array([2, 0], dtype=np.int32)), J(2), J(3))
    jinfo = S.longs(4)
    S.call("accmapFinish", None, J(h), jinfo)
    assert tuple(S.get(jinfo, 4)) == tuple(info)
    got = _jni_map(S, h, info[0], 3)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert S.call("accmapGetDevice", I, J(h)) == 0 and S.call("accmapGetNNodes", I, J(h)) == 3
    # lookups: header lines from the host, and those of a scanned chunk where the scan left them
    keys = ga.slot_accessions(want[0])
    headers = [b">" + k + b" x" for k in keys[::5]] + [b">NC_404 x", b">" + keys[0]]
    fasta = b"".join(hd + b"\n" + b"ACGTTGCA" * (3 + i % 4) + b"\n" for i, hd in enumerate(headers))
    for complete in (0, 1):
        want_nodes = m.lookup(headers, complete_only=bool(complete))
        off = np.concatenate([[0], np.cumsum([len(x) for x in headers])]).astype(np.uint64)
        raw = np.frombuffer(b"".join(headers), dtype=np.uint8)
        out = np.full(len(headers), -7, dtype=np.int32)
        S.call("accmapLookup", None, J(h), *S.buf(raw), *S.buf(off), J(len(headers)), Z(complete), *S.buf(out))
        assert np.array_equal(out, want_nodes) and (out >= 0).any() and (out < 0).any()
    assert SHORT in S.call("accmapLookup", None, J(h), *S.buf(raw[:-1]), *S.buf(off), J(len(headers)), Z(0), *S.buf(out), throws=True)
    g = ga.DeviceGenomes()
    g.scan(fasta)
    want_nodes = m.lookup_genomes(g, complete_only=True)
    keep = (want_nodes >= 0).astype(np.uint8)
    g.gather(keep)
    jg = S.call("genomesCreate", J, I(0))
    scan = S.longs(4)
    S.call("genomesScan", None, J(jg), *S.text(fasta), Z(1), scan)
    n_rec, used, hb, _ml = S.get(scan, 4)
    assert (n_rec, used, hb) == (len(headers), len(fasta), g.header_bytes) and n_rec == g.n_records
    hdr, hoff = np.zeros(hb, dtype=np.uint8), np.zeros(n_rec + 1, dtype=np.uint64)
    S.call("genomesHeaders", None, J(jg), *S.buf(hdr), *S.buf(hoff))
    assert hdr.tobytes() == b"".join(headers) and np.array_equal(hoff, off)
    out = np.full(n_rec, -7, dtype=np.int32)
    S.call("accmapLookupGenomes", None, J(h), J(jg), Z(1), *S.buf(out))
    assert np.array_equal(out, want_nodes)
    gathered = S.longs(2)
    S.call("genomesGather", None, J(jg), *S.buf(keep), gathered)
    assert S.get(gathered, 2) == [g.n_regions, g.n_bases] and 0 < g.n_regions < n_rec
    where = S.longs(2)
    S.call("genomesRegions", None, J(jg), where)
    assert all(S.get(where, 2))
    assert SHORT in S.call("genomesHeaders", None, J(jg), *S.buf(hdr), *S.buf(hoff[:-1]), throws=True)
    assert SHORT in S.call("accmapLookupGenomes", None, J(h), J(jg), Z(1), *S.buf(out[:-1]), throws=True)
    assert SHORT in S.call("accmapFetch", None, J(h), *S.buf(np.zeros(32 * info[0] - 1, dtype=np.uint8)), *S.buf(None), *S.buf(None), throws=True)
    S.call("genomesDestroy", None, J(jg))
    S.call("accmapDestroy", None, J(h))
    g.close()
    m.close()
    # the file-level call: the map, and the count alone
    path = tmp_path / "c.catalog"
    path.write_bytes(text)
    wm, wtot = host.accmap_files([path], KNOWN, CATS, STATS)
    want = wm.fetch()
    for count_only in (0, 1):
        tot = S.longs(5)
        h = S.call("hostAccmapFiles", J, S.strings([path]), I(0), Z(1), Z(0), Z(0), S.strings(CATS), S.strings(STATS), *S.buf(KNOWN), I(3), J(0), Z(count_only), tot)
        assert S.get(tot, 5) == [wtot[k] for k in ("lines", "passing", "put", "device_chunks", "host_chunks")]
        assert (h == 0) == bool(count_only)
        if h:
            for g_, w in zip(_jni_map(S, h, wtot["put"], 3), want):
                assert np.array_equal(g_, w)
            S.call("accmapDestroy", None, J(h))
    wm.close()
    msg = S.call("hostAccmapFiles", J, S.strings([tmp_path / "no_such.catalog"]), I(0), Z(1), Z(0), Z(0), S.strings(CATS), S.strings(STATS), *S.buf(KNOWN), I(3), J(0),
                 Z(0), S.longs(5), throws=True)
    assert b"no_such.catalog" in msg
    assert SHORT in S.call("accmapCreate", J, I(0), Z(1), Z(0), Z(0), S.strings(CATS), S.strings(STATS), *S.buf(KNOWN[:2]), I(3), J(0), throws=True)


# ---- asmsum
def _jni_picks(S, h, m):
    nodes, quality, is_ref, lines = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.int64)
    off = np.zeros(3 * m + 1, dtype=np.uint64)
    S.call("asmsumFetch", None, J(h), *S.buf(nodes), *S.buf(quality), *S.buf(is_ref), *S.buf(lines), *S.buf(off), *S.buf(None))
    pool = np.zeros(max(int(off[3 * m]), 1), dtype=np.uint8)
    S.call("asmsumFetch", None, J(h), *[x for _ in range(5) for x in S.buf(None)], *S.buf(pool))
    if int(off[3 * m]) > 1:
        assert SHORT in S.call("asmsumFetch", None, J(h), *[x for _ in range(5) for x in S.buf(None)], *S.buf(pool[:int(off[3 * m]) - 1]), throws=True)
    raw = pool.tobytes()
    s = lambda i: raw[int(off[i]):int(off[i + 1])]  # noqa: E731
    return [(int(nodes[j]), s(3 * j), s(3 * j + 1), s(3 * j + 2), int(quality[j]), bool(is_ref[j]), int(lines[j])) for j in range(m)]


def test_asmsum_natives(jni, tmp_path):
    S = jni
    text = asmsum.summary(300, KNOWN.tolist(), seed=3)
    flt = np.array([1, 0, 1], dtype=np.uint8)
    extra = [(2, b"3", b"3", b"https://host/path/GCA_1.1_X", 1, False, 10 ** 6)]
    a = ga.DeviceAssemblySummary(KNOWN, flt, qualities=None)
    r = a.submit(text, last=True)
    a.append(extra, n_counted=2, n_lines=3)
    info = a.finish(2)
    want = a.fetch()
    assert r["refused"] == 0 and info[1] >= 3
    h = S.call("asmsumCreate", J, I(0), *S.buf(KNOWN), I(3), *S.buf(flt), I(-1), Z(0), Z(0), J(0))
    rep = S.longs(8)
    S.call("asmsumSubmit", None, J(h), *S.text(text), Z(1), rep)
    assert S.get(rep, 8) == [r[k] for k in ("counted", "kept", "short", "refused", "first_bad_line", "longest_line", "skipped", "pool_bytes")]
    strs = [extra[0][1], extra[0][2], extra[0][3]]
    S.call("asmsumAppend", None, J(h), *S.buf(np.array([2], np.int32)), *S.buf(np.array([1], np.uint8)), *S.buf(np.array([0], np.uint8)),
           *S.buf(np.array([10 ** 6], np.int64)), *S.buf(np.concatenate([[0], np.cumsum([len(x) for x in strs])]).astype(np.uint64)),
           *S.buf(np.frombuffer(b"".join(strs), dtype=np.uint8)), J(1), J(2), J(3))
    jinfo = S.longs(4)
    S.call("asmsumFinish", None, J(h), I(2), jinfo)
    assert tuple(S.get(jinfo, 4)) == tuple(info)
    assert _jni_picks(S, h, info[1]) == want
    assert S.call("asmsumGetDevice", I, J(h)) == 0
    assert SHORT in S.call("asmsumFetch", None, J(h), *S.buf(np.zeros(info[1] - 1, np.int32)), *[x for _ in range(5) for x in S.buf(None)], throws=True)
    ftp = np.frombuffer(want[0][3], dtype=np.uint8)
    name = np.zeros(len(ftp) + 16, dtype=np.uint8)
    n = S.call("asmsumFileName", J, *S.buf(ftp), J(len(ftp)), *S.buf(name))
    assert name[:n].tobytes() == ga.file_name_of(want[0][3])
    assert SHORT in S.call("asmsumFileName", J, *S.buf(ftp), J(len(ftp) + 1), *S.buf(name), throws=True)
    S.call("asmsumDestroy", None, J(h))
    a.close()
    # the file-level call
    path = tmp_path / "assembly_summary.txt"
    path.write_bytes(text)
    picks, total, wtot = host.assembly_summary_files([path], KNOWN, selected=[0, 2], qualities=None, max_per_taxid=2)
    tot = S.longs(7)
    h = S.call("hostAsmsumFiles", J, S.strings([path]), I(0), *S.buf(KNOWN), I(3), *S.buf(flt), I(-1), Z(0), Z(0), J(0), I(2), tot)
    assert S.get(tot, 7) == [wtot[k] for k in ("lines", "counted", "kept", "picked", "nodes", "device_chunks", "host_chunks")]
    got = {}
    for node, taxid, species, ftp_, quality, is_ref, line in _jni_picks(S, h, wtot["picked"]):
        got.setdefault(node, []).append({"taxid": taxid, "species_taxid": species, "ftp_url": ftp_, "file_name": ga.file_name_of(ftp_),
                                         "quality": ga.ASSEMBLY_QUALITIES[quality], "is_reference": is_ref, "line": line})
    assert got == picks and len(picks) == 2
    S.call("asmsumDestroy", None, J(h))
    msg = S.call("hostAsmsumFiles", J, S.strings([tmp_path / "no_such_summary.txt"]), I(0), *S.buf(KNOWN), I(3), *S.buf(None), I(-1), Z(0), Z(0), J(0), I(1),
                 S.longs(7), throws=True)
    assert b"no_such_summary.txt" in msg


# ---- genome files straight into a handle
def test_host_genome_files_into(jni, tmp_path, monkeypatch):
    S = jni
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "256")
    paths, node_of_file = gi.collection(tmp_path)
    amap = gi.accession_map()
    base = gi.base_store(paths, node_of_file, amap)
    known = np.array(gi.KNOWN, dtype=np.int32)
    h = S.call("accmapCreate", J, I(0), Z(1), Z(0), Z(0), S.strings(["bacteria"]), S.strings(["REVIEWED"]), *S.buf(known), I(len(known)), J(0))
    S.call("accmapAppend", None, J(h), *S.buf(ga.accession_slots([k for k, _ in gi.MAP_ENTRIES])), *S.buf(np.array([n for _, n in gi.MAP_ENTRIES], dtype=np.int32)),
           J(len(gi.MAP_ENTRIES)), J(len(gi.MAP_ENTRIES)))
    S.call("accmapFinish", None, J(h), S.longs(4))
    kind_of = {"DeviceDbSizer": 0, "DeviceDbBuilder": 1, "DeviceDbUpdater": 2, "DeviceDbQuality": 3}

    def walk(target, update, paths_=paths, throws=False):
        tot = S.longs(7)
        got = S.call("hostGenomeFilesInto", None, S.strings(paths_), I(0), J(h), Z(1), S.ints(node_of_file), *S.buf(gi.VI_OF_NODE), I(len(gi.VI_OF_NODE)),
                     I(kind_of[type(target).__name__]), J(target.h.value), Z(int(update)), tot, throws=throws)
        if throws:
            return got
        v = S.get(tot, 7)
        return types.SimpleNamespace(records=v[0], kept_records=v[1], text_bytes=v[2], kept_bases=v[3], chunks=v[4], host_chunks=v[5], max_line_bytes=v[6])

    for kind in gi.KINDS:
        want, want_tot = gi.drive(kind, gi.through_callbacks(paths, node_of_file, amap), base)
        got, got_tot = gi.drive(kind, walk, base)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), kind
        assert got_tot == want_tot and got_tot[0][:2] == (13, 9), (kind, got_tot, want_tot)
    b = ga.DeviceDbBuilder(gi.K, len(gi.PARENT_VI), gi.PARENT_VI)
    assert SHORT in S.call("hostGenomeFilesInto", None, S.strings(paths), I(0), J(h), Z(1), S.ints(node_of_file), *S.buf(gi.VI_OF_NODE[:3]), I(4), I(1), J(b.h.value),
                           Z(0), S.longs(7), throws=True)
    assert SHORT in S.call("hostGenomeFilesInto", None, S.strings(paths), I(0), J(h), Z(1), S.ints(node_of_file[:3]), *S.buf(gi.VI_OF_NODE), I(4), I(1), J(b.h.value),
                           Z(0), S.longs(7), throws=True)
    msg = walk(b, False, paths_=[paths[0], str(tmp_path / "no_such_genome.fna"), paths[2], paths[3]], throws=True)
    assert b"no_such_genome.fna" in msg
    # an argument error of the call itself comes back as the host layer's message
    msg = S.call("hostGenomeFilesInto", None, S.strings(paths), I(0), J(0), Z(1), S.ints(node_of_file), *S.buf(gi.VI_OF_NODE), I(4), I(1), J(b.h.value), Z(0),
                 S.longs(7), throws=True)
    assert b"accession map" in msg and SHORT not in msg
    b.close()
    S.call("accmapDestroy", None, J(h))
    amap.close()
