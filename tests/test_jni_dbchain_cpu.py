"""The natives of the database-construction chain without a device: host-only handles (device -1) of the taxtree, accmap and asmsum
families through java/jni/gsgpu_jni.c on the functional JNIEnv of tests/native/jni_stub, held to the ctypes path over the same
handles, and the refusals that come before the C ABI is entered -- a stated capacity that is too small, a handle of 0, a fetch in
front of finish.  The device paths are tested on the GPU (tests/test_gpu_jni_dbchain.py)."""
import numpy as np
import pytest

import genestrip_amd as ga
import taxtree_cases
from jnishim import I, J, SHORT, Z, build

KNOWN = np.array([7, 562, 9606, 10090], dtype=np.int32)


@pytest.fixture(scope="module")
def jni(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("jni") / "libgsjni_cpu.so"))


def test_host_only_tree(jni):
    S = jni
    dump = taxtree_cases.random_dump(120, 5)
    t = ga.DeviceTaxTree(device=-1)
    t.append_nodes(dump, last=True)
    info = t.finish()
    want = t.arrays()
    n = t.n_nodes
    h = S.call("taxtreeCreate", J, I(-1))
    assert S.call("taxtreeGetDevice", I, J(h)) == -1
    rep = S.longs(8)
    assert b"gsgpu error" in S.call("taxtreeFetch", None, J(h), *[x for _ in range(6) for x in S.buf(np.zeros(4, dtype=np.int32))], throws=True)
    S.call("taxtreeAppendNodes", None, J(h), *S.text(dump), Z(1), rep)
    jinfo = S.longs(8)
    S.call("taxtreeFinishNodes", None, J(h), jinfo)
    assert S.get(jinfo, 2) == [info["nodes"], info["reached"]]
    out = {k: np.full(n, -7, dtype=np.int32) for k in ("taxids", "parent", "depth", "position", "subtree", "rank")}
    S.call("taxtreeFetch", None, J(h), *[x for k in out for x in S.buf(out[k])])
    for k in out:
        assert np.array_equal(out[k], want[k]), k
    sel = np.zeros(n, dtype=np.uint8)
    count = S.call("taxtreeSelect", J, J(h), S.ints([0]), J(1), S.ints([n // 2]), J(1), I(-1), *S.buf(sel))
    want_sel = t.select([0], [n // 2])
    assert np.array_equal(sel, want_sel) and count == int(want_sel.sum()) > 0
    regions = (np.arange(n, dtype=np.int32) * 3) % 4
    selected = np.flatnonzero(want_sel).astype(np.int32)
    want_below, want_incl = t.regions_below(regions, selected, 6)
    incl, below = np.zeros(n, dtype=np.int32), np.zeros(len(selected), dtype=np.int32)
    n_below = S.call("taxtreeRegionsBelow", J, J(h), *S.buf(regions), S.ints(selected), J(len(selected)), I(6), I(-1), *S.buf(incl), *S.buf(below))
    assert np.array_equal(incl, want_incl) and np.array_equal(below[:n_below], want_below)
    want_small = t.small_tree(regions)
    outs = [np.zeros(max(t.n_reached, 1), dtype=np.int32) for _ in range(4)]
    n_small = S.call("taxtreeSmall", I, J(h), *S.buf(regions), I(4), *[x for o in outs for x in S.buf(o)])
    assert n_small == len(want_small["node_of_vi"]) and np.array_equal(outs[1][:n_small], want_small["parent_vi"])
    # refusals in front of the C ABI
    assert SHORT in S.call("taxtreeFetch", None, J(h), *S.buf(out["taxids"][:-1]), *[x for _ in range(5) for x in S.buf(None)], throws=True)
    assert SHORT in S.call("taxtreeSelect", J, J(h), S.ints([0]), J(2), None, J(0), I(-1), *S.buf(sel), throws=True)
    assert SHORT in S.call("taxtreeSelect", J, J(h), S.ints([0]), J(1), None, J(0), I(-1), *S.buf(sel[:-1]), throws=True)
    assert SHORT in S.call("taxtreeRegionsBelow", J, J(h), *S.buf(regions[:-1]), S.ints(selected), J(len(selected)), I(6), I(-1), *S.buf(None), *S.buf(None), throws=True)
    assert SHORT in S.call("taxtreeSmall", I, J(h), *S.buf(regions), I(2), *[x for _ in range(4) for x in S.buf(None)], throws=True)
    assert SHORT in S.call("taxtreeAppendNodes", None, J(h), *S.buf(np.zeros(8, dtype=np.uint8)), J(9), Z(1), rep, throws=True)
    assert SHORT in S.call("taxtreeFinishNodes", None, J(h), S.longs(7), throws=True)
    assert SHORT in S.call("taxtreeFetch", None, J(0), *[x for _ in range(6) for x in S.buf(None)], throws=True)
    S.call("taxtreeDestroy", None, J(h))
    S.call("taxtreeDestroy", None, J(0))
    t.close()
    req, exc, counts = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.int32), S.longs(2)
    S.call("taxtreeReadTaxids", None, *S.text(taxtree_cases.TAXIDS_TEXT), *S.buf(req), *S.buf(exc), J(16), counts)
    n_req, n_exc = S.get(counts, 2)
    assert (req[:n_req].tolist(), exc[:n_exc].tolist()) == tuple(taxtree_cases.TAXIDS_NUMBERS)
    assert SHORT in S.call("taxtreeReadTaxids", None, *S.text(taxtree_cases.TAXIDS_TEXT), *S.buf(req), *S.buf(exc[:4]), J(16), counts, throws=True)


def test_host_only_accession_map(jni):
    S = jni
    keys = [b"NC_000002.1", b"NZ_AB01.1", b"NC_000001.7", b"NC_000002.1", b"WP_3.1"]
    nodes = np.array([1, 0, 3, 2, 1], dtype=np.int32)
    m = ga.DeviceAccessionMap(KNOWN, ["bacteria"], ["REVIEWED"], device=-1)
    m.append(keys, nodes, n_passing=7)
    info = m.finish()
    want = m.fetch()
    h = S.call("accmapCreate", J, I(-1), Z(1), Z(0), Z(0), S.strings(["bacteria"]), S.strings(["REVIEWED"]), *S.buf(KNOWN), I(4), J(0))
    assert (S.call("accmapGetDevice", I, J(h)), S.call("accmapGetNNodes", I, J(h))) == (-1, 4)
    assert b"gsgpu error" in S.call("accmapFetch", None, J(h), *S.buf(None), *S.buf(None), *S.buf(np.zeros(4, dtype=np.int32)), throws=True)
    slots = ga.accession_slots(keys)
    assert SHORT in S.call("accmapAppend", None, J(h), *S.buf(slots[:-1]), *S.buf(nodes), J(5), J(7), throws=True)
    assert SHORT in S.call("accmapAppend", None, J(h), *S.buf(slots), *S.buf(nodes[:-1]), J(5), J(7), throws=True)
    S.call("accmapAppend", None, J(h), *S.buf(slots), *S.buf(nodes), J(5), J(7))
    jinfo = S.longs(4)
    S.call("accmapFinish", None, J(h), jinfo)
    assert tuple(S.get(jinfo, 4)) == tuple(info) and info[0] == 5 and info[1] == 7 and info[2] == 1
    got = np.zeros((5, 32), dtype=np.uint8), np.zeros(5, dtype=np.int32), np.zeros(4, dtype=np.int32)
    S.call("accmapFetch", None, J(h), *S.buf(got[0]), *S.buf(got[1]), *S.buf(got[2]))
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    headers = [b">NC_000002.1 first in the input wins", b">WP_3.1 x", b">NC_000001.7", b">NC_9 x"]
    off = np.concatenate([[0], np.cumsum([len(x) for x in headers])]).astype(np.uint64)
    raw = np.frombuffer(b"".join(headers), dtype=np.uint8)
    for complete in (0, 1):
        out = np.full(4, -7, dtype=np.int32)
        S.call("accmapLookup", None, J(h), *S.buf(raw), *S.buf(off), J(4), Z(complete), *S.buf(out))
        assert out.tolist() == m.lookup(headers, complete_only=bool(complete)).tolist() == [1, -1 if complete else 1, -1, -1]
    assert SHORT in S.call("accmapLookup", None, J(h), *S.buf(raw), *S.buf(off), J(4), Z(0), *S.buf(out[:-1]), throws=True)
    assert SHORT in S.call("accmapLookup", None, J(h), *S.buf(raw[:-1]), *S.buf(off), J(4), Z(0), *S.buf(out), throws=True)
    assert SHORT in S.call("accmapLookup", None, J(h), *S.buf(raw), *S.buf(off[:-1]), J(4), Z(0), *S.buf(out), throws=True)
    assert SHORT in S.call("accmapFetch", None, J(h), *S.buf(None), *S.buf(None), *S.buf(got[2][:-1]), throws=True)
    assert SHORT in S.call("accmapCreate", J, I(-1), Z(1), Z(0), Z(0), S.strings(["bacteria"]), S.strings(["REVIEWED"]), *S.buf(KNOWN[:3]), I(4), J(0), throws=True)
    # hostGenomeFilesInto: what the shim refuses, and an argument error of the call itself as the host layer's message
    vi = np.array([0, 1, 2, 3], dtype=np.int32)
    dummy = np.zeros(4, dtype=np.int64)
    args = lambda vi_, n_nodes, nof, am=h: (S.strings(["a.fna", "b.fna"]), I(0), J(am), Z(0), nof, *S.buf(vi_), I(n_nodes), I(1), J(dummy.ctypes.data), Z(0), S.longs(7))  # noqa: E731
    assert SHORT in S.call("hostGenomeFilesInto", None, *args(vi[:3], 4, None), throws=True)
    assert SHORT in S.call("hostGenomeFilesInto", None, *args(vi, 4, S.ints([0])), throws=True)
    msg = S.call("hostGenomeFilesInto", None, *args(vi[:3], 3, None), throws=True)
    assert b"gsgpu error -1" in msg and b"3 nodes" in msg
    msg = S.call("hostGenomeFilesInto", None, *args(vi, 4, S.ints([0, -1]), am=0), throws=True)
    assert b"gsgpu error -1" in msg and b"file 1" in msg
    S.call("accmapDestroy", None, J(h))
    m.close()


def test_host_only_assembly_summary(jni):
    S = jni
    entries = [(1, b"562", b"562", b"https://h/p/GCA_1.1_A", 3, False, 4), (1, b"562", b"561", b"https://h/p/GCA_2.1_B/", 1, True, 9),
               (3, b"10090", b"10090", b"https://h/p/GCA_3.2_C", 1, False, 11), (1, b"562", b"562", b"https://h/p/GCA_4.1_D", 2, False, 12)]
    a = ga.DeviceAssemblySummary(KNOWN, None, qualities=None, device=-1)
    a.append(entries, n_counted=6, n_lines=13)
    info = a.finish(2)
    want = a.fetch()
    h = S.call("asmsumCreate", J, I(-1), *S.buf(KNOWN), I(4), *S.buf(None), I(-1), Z(0), Z(0), J(0))
    assert S.call("asmsumGetDevice", I, J(h)) == -1
    strs = [s for e in entries for s in (e[1], e[2], e[3])]
    cols = (np.array([e[0] for e in entries], np.int32), np.array([e[4] for e in entries], np.uint8), np.array([e[5] for e in entries], np.uint8),
            np.array([e[6] for e in entries], np.int64), np.concatenate([[0], np.cumsum([len(x) for x in strs])]).astype(np.uint64),
            np.frombuffer(b"".join(strs), dtype=np.uint8))
    for short in range(6):
        bufs = [x for i, c in enumerate(cols) for x in S.buf(c[:-1] if i == short else c)]
        assert SHORT in S.call("asmsumAppend", None, J(h), *bufs, J(4), J(6), J(13), throws=True)
    S.call("asmsumAppend", None, J(h), *[x for c in cols for x in S.buf(c)], J(4), J(6), J(13))
    assert b"gsgpu error" in S.call("asmsumFetch", None, J(h), *[x for _ in range(6) for x in S.buf(None)], throws=True)
    jinfo = S.longs(4)
    S.call("asmsumFinish", None, J(h), I(2), jinfo)
    assert tuple(S.get(jinfo, 4)) == tuple(info) and info[0] == 4 and info[1] == 3
    m = info[1]
    nodes, quality, is_ref, lines = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.uint8), np.zeros(m, np.int64)
    off = np.zeros(3 * m + 1, dtype=np.uint64)
    S.call("asmsumFetch", None, J(h), *S.buf(nodes), *S.buf(quality), *S.buf(is_ref), *S.buf(lines), *S.buf(off), *S.buf(None))
    pool = np.zeros(int(off[3 * m]), dtype=np.uint8)
    S.call("asmsumFetch", None, J(h), *[x for _ in range(5) for x in S.buf(None)], *S.buf(pool))
    raw = pool.tobytes()
    s = lambda i: raw[int(off[i]):int(off[i + 1])]  # noqa: E731
    assert [(int(nodes[j]), s(3 * j), s(3 * j + 1), s(3 * j + 2), int(quality[j]), bool(is_ref[j]), int(lines[j])) for j in range(m)] == want
    assert SHORT in S.call("asmsumFetch", None, J(h), *[x for _ in range(5) for x in S.buf(None)], *S.buf(pool[:-1]), throws=True)
    assert SHORT in S.call("asmsumFetch", None, J(h), *[x for _ in range(4) for x in S.buf(None)], *S.buf(off[:-1]), *S.buf(None), throws=True)
    ftp = np.frombuffer(entries[1][3], dtype=np.uint8)
    name = np.zeros(64, dtype=np.uint8)
    n = S.call("asmsumFileName", J, *S.buf(ftp), J(len(ftp)), *S.buf(name))
    assert name[:n].tobytes() == ga.file_name_of(entries[1][3]) == b"GCA_2.1_B_genomic.fna.gz"
    S.call("asmsumDestroy", None, J(h))
    a.close()
