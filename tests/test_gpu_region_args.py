"""gs_dbbuild, gs_dbquality and gs_dbupdate take the same input -- a batch of regions (seq, offsets, one tag per region, mem) --
and their begins take the same parameters.  One table of defective batches goes through ctypes to all three _add functions, one
table of defective parameters to every begin: each case pins the return code and the exact gs_last_error() text, shows that the
refused call left the handle as it was, and that the handle then gives the result of a handle that never saw the defect.
Needs an MI355X: run with -m gpu."""
import ctypes as C
import types

import numpy as np
import pytest

import genestrip_amd as ga
import qualitycheck as qc
import test_gpu_build as tbuild
import test_gpu_dbquality as tquality
import test_gpu_dbupdate as tupdate

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, STATE = 0, -1, -4, -5
PARENT = tupdate.PARENT  # seven nodes and value 7 without a tree node
assert np.array_equal(PARENT, tquality.PARENT) and np.array_equal(PARENT[:7], tbuild.PARENT)
NV = len(PARENT)
K = 21
FAMILIES = ("build", "quality", "update")
WHOLE = (0, 2 ** 64 - 1)  # the range every handle starts with

BAD_ARGUMENT = "bad argument"
BAD_MEM = "mem must be GS_MEM_HOST or GS_MEM_DEVICE"
OFF_FIRST = "offsets[0] must be 0"
OFF_ORDER = "offsets must not decrease"
NOT_A_NODE = "node_vi: not a node of the tree"
NOT_A_VALUE = "leaf_vi: not a value of the store"
BAD_K = "k must be in [1,31]"
BAD_TREE = "bad tree arrays (n_values must be in [1, 2^24])"
BAD_STEP = "stepSize must be >= 1 (C/GSConfigKey.java:236)"
BAD_DUST = "maxDust > Short.MAX_VALUE (C/util/CGATLongBuffer.java:78-80)"
ONE_ROOT = "{who} needs a tree with exactly one root"
STRIPE = "{who} needs the whole store on one device: this handle is a stripe"


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _last_error():
    return (ga.lib().gs_last_error() or b"").decode()


@pytest.fixture(scope="module")
def case():
    fill, update = tupdate._regions(K, 1, 4242, n=12)
    kmers, vals, _ = tupdate._oracle(K, fill, [], PARENT)
    seq, off = qc.pack([s for s, _ in update])
    tags = np.array([n for _, n in update], dtype=np.int32)
    assert len(tags) >= 4 and off[1] > 0  # (the defects below are written into regions 1 and 2)
    store = ga.DeviceKMerStore(K, kmers, vals, NV, PARENT)
    c = types.SimpleNamespace(kmers=kmers, vals=vals, store=store, seq=seq, off=off, tags=tags, n=len(tags))
    c.clean = {}
    for family in FAMILIES:  # what a handle that sees the good batch only gives
        h = _open(family, c)
        assert _add(family, h, seq, off, tags, c.n, ga.MEM_HOST) == OK, _last_error()
        c.clean[family] = _result(family, h)
        h.close()
    assert len(c.clean["build"][0]) > 0 and c.clean["quality"][1].any() and c.clean["update"][2] > 0
    yield c
    store.close()


def _open(family, c):
    if family == "build":
        return ga.DeviceDbBuilder(K, NV, PARENT)
    if family == "quality":
        return ga.DeviceDbQuality(c.store)
    return ga.DeviceDbUpdater.from_arrays(K, c.kmers, c.vals, NV, PARENT)


def _add(family, h, seq, off, tags, n, mem):
    L = ga.lib()
    if family == "build":
        return L.gs_dbbuild_add(h.h, _p(seq), _p(off), _p(tags), n, mem, 0)
    return getattr(L, f"gs_db{family}_add")(h.h, _p(seq), _p(off), _p(tags), n, mem)


def _result(family, h):
    if family == "update":
        moved = h.finish()
        return h.fetch() + (moved,)
    return h.finish()


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _untouched(family, h):
    """nothing has been added to this handle"""
    L = ga.lib()
    if family == "update":
        st = h.stats()
        return st.n_pairs == 0 and st.n_found == 0 and st.n_moved == 0 and st.batch_bytes_peak == 0
    return getattr(L, f"gs_db{family}_set_range")(h.h, *WHOLE) == OK  # (refused once a pass has regions)


def _with(c, **change):
    """the good batch with one or more fields replaced -> the arguments of _add behind the handle"""
    a = dict(seq=c.seq, off=c.off, tags=c.tags, n=c.n, mem=ga.MEM_HOST)
    a.update(change)
    return a["seq"], a["off"], a["tags"], a["n"], a["mem"]


def _tag(c, v):
    t = c.tags.copy()
    t[1] = v
    return t


def _off_first(c):
    return c.off + np.uint64(1)


def _off_decreasing(c):
    o = c.off.copy()
    o[2] = o[1] - np.uint64(1)
    return o


# name, the batch, (code, message) of build and update, (code, message) of quality
DEFECTS = [
    ("bad mem", lambda c: _with(c, mem=7), (INVALID, BAD_MEM), (INVALID, BAD_MEM)),
    ("offsets[0] != 0", lambda c: _with(c, off=_off_first(c)), (INVALID, OFF_FIRST), (INVALID, OFF_FIRST)),
    ("decreasing offsets", lambda c: _with(c, off=_off_decreasing(c)), (INVALID, OFF_ORDER), (INVALID, OFF_ORDER)),
    ("a tag of n_values", lambda c: _with(c, tags=_tag(c, NV)), (INVALID, NOT_A_NODE), (INVALID, NOT_A_VALUE)),
    ("a tag without a node", lambda c: _with(c, tags=_tag(c, 7)), (INVALID, NOT_A_NODE), None),  # quality: see below
    ("a negative tag", lambda c: _with(c, tags=_tag(c, -1)), (INVALID, NOT_A_NODE), None),
    ("NULL seq", lambda c: _with(c, seq=None), (INVALID, BAD_ARGUMENT), (INVALID, BAD_ARGUMENT)),
    ("NULL offsets", lambda c: _with(c, off=None), (INVALID, BAD_ARGUMENT), (INVALID, BAD_ARGUMENT)),
    ("NULL tags", lambda c: _with(c, tags=None), (INVALID, BAD_ARGUMENT), (INVALID, BAD_ARGUMENT)),
    ("negative n_regions", lambda c: _with(c, n=-1), (INVALID, BAD_ARGUMENT), (INVALID, BAD_ARGUMENT)),
    # several defects in one call: mem, then tags, then offsets
    ("bad mem and a bad tag", lambda c: _with(c, mem=7, tags=_tag(c, NV)), (INVALID, BAD_MEM), (INVALID, BAD_MEM)),
    ("bad mem and bad offsets", lambda c: _with(c, mem=-1, off=_off_first(c)), (INVALID, BAD_MEM), (INVALID, BAD_MEM)),
    ("a bad tag and bad offsets", lambda c: _with(c, tags=_tag(c, NV), off=_off_decreasing(c)), (INVALID, NOT_A_NODE), (INVALID, NOT_A_VALUE)),
]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,batch,node_family,leaf_family", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_a_defective_batch_is_refused_and_changes_nothing(case, family, name, batch, node_family, leaf_family):
    want = leaf_family if family == "quality" else node_family
    h = _open(family, case)
    if want is None:
        # gs_dbquality: a region whose tag has no node counts nothing (leafNode == null); the other regions count as before
        assert _add(family, h, *batch(case)) == OK, _last_error()
        counts, present = h.finish()
        seq, off, tags, n, mem = batch(case)
        keep = [i for i in range(n) if i != 1]
        h2 = _open(family, case)
        s2, o2 = qc.pack([bytes(seq[int(off[i]):int(off[i + 1])]) for i in keep])
        assert _add(family, h2, s2, o2, np.ascontiguousarray(tags[keep]), len(keep), mem) == OK, _last_error()
        assert _same((counts, present), h2.finish())
        assert not present[7] and not counts[7].any()
        h2.close()
    else:
        rc = _add(family, h, *batch(case))
        assert (rc, _last_error()) == want
        assert _untouched(family, h)
        assert _add(family, h, *_with(case)) == OK, _last_error()
        assert _same(_result(family, h), case.clean[family])
    h.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_a_batch_of_only_tags_without_a_node(case, family):
    """every region of the batch carries value 7: build and update refuse it, quality counts nothing at all"""
    h = _open(family, case)
    rc = _add(family, h, *_with(case, tags=np.full(case.n, 7, np.int32)))
    if family == "quality":
        assert rc == OK, _last_error()
        counts, present = h.finish()
        assert not present.any() and not counts.any()
    else:
        assert (rc, _last_error()) == (INVALID, NOT_A_NODE)
        assert _untouched(family, h)
    h.close()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("pointers", [True, False])
def test_no_regions_is_ok_and_changes_nothing(case, family, pointers):
    h = _open(family, case)
    args = _with(case, n=0) if pointers else (None, None, None, 0, ga.MEM_HOST)
    assert _add(family, h, *args) == OK
    assert _add(family, h, *args[:4], 7) == OK  # (nothing is looked at: not even mem)
    assert _untouched(family, h)
    assert _add(family, h, *_with(case)) == OK, _last_error()
    assert _same(_result(family, h), case.clean[family])
    h.close()
    h = _open(family, case)
    assert _add(family, h, *args) == OK
    empty = _result(family, h)
    if family == "build":
        assert len(empty[0]) == 0 and len(empty[1]) == 0
    elif family == "quality":
        assert not empty[0].any() and not empty[1].any() and h.stats().n_pairs == 0
    else:
        assert np.array_equal(empty[0], case.kmers) and np.array_equal(empty[1], case.vals) and empty[2] == 0
    h.close()


TWO_ROOTS = np.array([-1, 0, 1, 1, 2, 4, -1, -2], dtype=np.int32)

# name, the parameters that differ from a good begin, code, message
BEGIN_DEFECTS = [
    ("k 0", dict(k=0), INVALID, BAD_K),
    ("k 32", dict(k=32), INVALID, BAD_K),
    ("n_values 0", dict(n_values=0), INVALID, BAD_TREE),
    ("NULL parent_vi", dict(parent=None), INVALID, BAD_TREE),
    ("step_size 0", dict(step=0), INVALID, BAD_STEP),
    ("max_dust 32768", dict(max_dust=32768), INVALID, BAD_DUST),
    ("two roots", dict(parent=TWO_ROOTS), UNSUPPORTED, ONE_ROOT),
]


def _begin(family, out, k=K, n_values=NV, parent=PARENT, lower=1, max_dust=-1, step=1):
    L = ga.lib()
    if family == "build":
        return L.gs_dbbuild_begin(out, 0, k, n_values, _p(parent), lower, max_dust, step)
    return L.gs_dbupdate_begin(out, 0, k, n_values, _p(parent), lower, max_dust, step, None, None, 0, ga.MEM_HOST)


@pytest.mark.parametrize("family", ["build", "update"])
@pytest.mark.parametrize("name,change,code,message", BEGIN_DEFECTS, ids=[d[0] for d in BEGIN_DEFECTS])
def test_defective_parameters_are_refused_by_the_begins_that_take_a_tree(family, name, change, code, message):
    L = ga.lib()
    h = C.c_void_p(1)
    rc = _begin(family, C.byref(h), **change)
    assert (rc, _last_error()) == (code, message.format(who=f"gs_db{family}"))
    assert not h.value
    assert _begin(family, None) == INVALID and _last_error() == "out is NULL"
    assert _begin(family, C.byref(h)) == OK, _last_error()  # the good begin of this table
    assert getattr(L, f"gs_db{family}_destroy")(h) == OK


@pytest.mark.parametrize("family", ["quality", "update"])
def test_defective_parameters_are_refused_by_the_begins_that_take_a_store(case, family):
    L = ga.lib()
    begin = L.gs_dbquality_begin if family == "quality" else L.gs_dbupdate_begin_db
    who = f"gs_db{family}"
    h = C.c_void_p(1)
    for args, code, message in (((1, -1, 0), INVALID, BAD_STEP), ((1, 32768, 1), INVALID, BAD_DUST), ((0, 40000, -3), INVALID, BAD_STEP)):
        h.value = 1
        assert (begin(C.byref(h), case.store.h, *args), _last_error()) == (code, message)
        assert not h.value
    assert (begin(C.byref(h), None, 1, -1, 1), _last_error()) == (INVALID, "db is NULL")
    assert (begin(None, case.store.h, 1, -1, 1), _last_error()) == (INVALID, "out is NULL")
    stripe = ga.DeviceKMerStore.stripe(K, case.kmers, case.vals, NV, PARENT, device=0, n_stripes=2, stripe=0)
    h.value = 1
    assert (begin(C.byref(h), stripe.h, 1, -1, 1), _last_error()) == (UNSUPPORTED, STRIPE.format(who=who))
    assert not h.value
    stripe.close()
    assert begin(C.byref(h), case.store.h, 1, 32767, 1) == OK, _last_error()  # Short.MAX_VALUE itself is taken
    assert getattr(L, f"gs_db{family}_destroy")(h) == OK
