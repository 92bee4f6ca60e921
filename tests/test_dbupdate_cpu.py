"""gs_dbupdate (a finished store updated in batches, the reference's updatedb stage) without a GPU: the symbols exist and are
bound, and every bad argument is refused with GS_E_INVALID before a device is touched (on a machine without a GPU anything that
got as far as the device would answer GS_E_NODEVICE instead)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import genestrip_amd as ga
from genestrip_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gs_dbupdate_begin", "gs_dbupdate_begin_db", "gs_dbupdate_begin_build", "gs_dbupdate_set_slice", "gs_dbupdate_add",
           "gs_dbupdate_finish", "gs_dbupdate_fetch", "gs_dbupdate_to_db", "gs_dbupdate_get_stats", "gs_dbupdate_destroy")
PARENT = np.array([-1, 0, 1, 1, 2, 4, 0], dtype=np.int32)
INVALID, UNSUPPORTED = -1, -4


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gsgpu.h")).read()
    declared = set(re.findall(r"\b(gs_dbupdate_[a-z_0-9]+)\s*\(", header))
    assert declared == set(SYMBOLS)
    L = ga.lib()
    for name in SYMBOLS:
        assert name in ga.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert ga.abi_version() == 3  # additive change
    assert ga.DeviceDbUpdater is binding.DeviceDbUpdater
    for m in ("from_arrays", "from_store", "from_builder", "add", "set_slice", "finish", "fetch", "to_store", "stats", "close"):
        assert callable(getattr(ga.DeviceDbUpdater, m)), m


def test_stats_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "gsgpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gs_dbupdate_stats;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int64_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    want = [(n, "int64_t" if t is C.c_int64 else "double") for n, t in binding.DbUpdateStats._fields_]
    assert fields == want


def _begin(k=31, n_values=7, parent=PARENT, lower=1, max_dust=-1, step=1, kmers=None, vals=None, n=0, mem=ga.MEM_HOST, out=True):
    h = C.c_void_p()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = ga.lib().gs_dbupdate_begin(C.byref(h) if out else None, 0, k, n_values, p(parent), lower, max_dust, step, p(kmers), p(vals), n, mem)
    assert not h.value
    return rc


def test_begin_refuses_bad_arguments_before_any_device():
    kmers = np.array([5, 9], np.int64)
    vals = np.array([1, 2], np.int32)
    assert _begin(out=False) == INVALID
    assert _begin(k=0) == INVALID and _begin(k=32) == INVALID
    assert _begin(n_values=0) == INVALID
    assert _begin(parent=None) == INVALID
    assert _begin(step=0) == INVALID
    assert _begin(max_dust=40000) == INVALID
    assert _begin(n=-1) == INVALID
    assert _begin(kmers=None, vals=vals, n=2) == INVALID
    assert _begin(kmers=kmers, vals=None, n=2) == INVALID
    assert _begin(kmers=kmers, vals=vals, n=2, mem=7) == INVALID
    assert _begin(n_values=3, parent=np.array([-1, 2, 1], np.int32)) == INVALID  # a cycle
    assert _begin(n_values=3, parent=np.array([-1, 5, 0], np.int32)) == INVALID  # out of range
    assert _begin(n_values=3, parent=np.array([-1, -1, 0], np.int32)) == UNSUPPORTED  # a forest, as the builder refuses it
    assert b"one root" in ga.lib().gs_last_error()


def test_the_other_calls_refuse_null_handles():
    L = ga.lib()
    h = C.c_void_p()
    n = C.c_int64(0)
    st = binding.DbUpdateStats()
    assert L.gs_dbupdate_begin_db(None, None, 1, -1, 1) == INVALID
    assert L.gs_dbupdate_begin_db(C.byref(h), None, 1, -1, 1) == INVALID and not h.value
    assert L.gs_dbupdate_begin_build(None, None) == INVALID
    assert L.gs_dbupdate_begin_build(C.byref(h), None) == INVALID and not h.value
    assert L.gs_dbupdate_set_slice(None, 1000) == INVALID
    assert L.gs_dbupdate_add(None, None, None, None, 0, ga.MEM_HOST) == INVALID
    assert L.gs_dbupdate_finish(None, C.byref(n)) == INVALID
    assert L.gs_dbupdate_fetch(None, None, None) == INVALID
    assert L.gs_dbupdate_to_db(None, C.byref(h)) == INVALID
    assert L.gs_dbupdate_get_stats(None, C.byref(st)) == INVALID
    assert L.gs_dbupdate_destroy(None) == 0
    assert L.gs_last_error()


def test_python_wrapper_checks_lengths_first():
    with pytest.raises(ValueError):
        ga.DeviceDbUpdater.from_arrays(31, np.array([1, 2], np.int64), np.array([0], np.int32), 7, PARENT)
    with pytest.raises(ValueError):
        ga.DeviceDbUpdater.from_arrays(31, np.array([1], np.int64), np.array([0], np.int32), 7, PARENT[:3])
    with pytest.raises(TypeError):
        ga.DeviceDbUpdater()
