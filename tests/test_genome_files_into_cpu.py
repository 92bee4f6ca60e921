"""gs_host_genome_files_into: every argument error is GS_E_INVALID before any device call -- there is no device here -- and
gs_accmap_get_n_nodes, which the check of the table's length rests on.  The call itself is tested on the GPU
(tests/test_gpu_genome_files_into.py)."""
import ctypes as C

import numpy as np
import pytest

import genestrip_amd as ga
from genestrip_amd import host

INVALID = -1  # GS_E_INVALID
KNOWN = [7, 562, 9606, 10090]


@pytest.fixture(scope="module")
def amap():
    m = ga.DeviceAccessionMap(KNOWN, ["bacteria"], ["REVIEWED"], device=-1)  # host-only: touches no device
    m.append([b"NC_000001.1"], [0])
    m.finish()
    yield m
    m.close()


def _call(paths=("a.fna", "b.fna"), am=None, node_of_file=None, vi_of_node=(0, 1, 2, 3), n_nodes=None, kind=host.INTO_BUILD, handle=True,
          null_paths=False):
    """the raw call: no file of `paths` exists and `handle` points at nothing a library could use -- a check that came too late
    would show as another code, or not come back"""
    L = host.lib()
    arr = (C.c_char_p * max(len(paths), 1))(*[p.encode() for p in paths])
    vi = np.asarray(vi_of_node, dtype=np.int32)
    nof = None if node_of_file is None else np.asarray(node_of_file, dtype=np.int32)
    dummy = (C.c_int64 * 4)()
    tot = host.GenomeTotals()
    rc = L.gs_host_genome_files_into(None if null_paths else arr, len(paths), 0, am.h if am is not None else None, 0,
                                     None if nof is None else nof.ctypes.data_as(C.c_void_p), vi.ctypes.data_as(C.c_void_p) if len(vi) else None,
                                     len(vi) if n_nodes is None else n_nodes, kind, C.addressof(dummy) if handle else None, 0, C.byref(tot))
    return rc, (L.gs_host_last_error() or b"").decode()


def test_map_says_how_many_nodes_it_has(amap):
    n = C.c_int32(-1)
    assert ga.lib().gs_accmap_get_n_nodes(amap.h, C.byref(n)) == 0 and n.value == len(KNOWN)
    assert ga.lib().gs_accmap_get_n_nodes(None, C.byref(n)) == INVALID and ga.lib().gs_accmap_get_n_nodes(amap.h, None) == INVALID


def test_a_file_that_needs_a_lookup_without_a_map():
    rc, msg = _call()  # no node_of_file at all: every file needs one
    assert rc == INVALID and "file 0" in msg and "accession map" in msg
    rc, msg = _call(node_of_file=[2, -1])
    assert rc == INVALID and "file 1" in msg


def test_a_table_of_another_length_than_the_maps(amap):
    for vi in ((0, 1, 2), (0, 1, 2, 3, 3)):
        rc, msg = _call(am=amap, vi_of_node=vi)
        assert rc == INVALID and "%d nodes" % len(vi) in msg and "map 4" in msg


def test_an_unknown_kind(amap):
    for kind in (-1, 4, 99):
        rc, msg = _call(am=amap, kind=kind)
        assert rc == INVALID and "kind %d" % kind in msg


def test_null_handles_and_arrays(amap):
    assert _call(am=amap, handle=False)[0] == INVALID
    assert _call(am=amap, null_paths=True)[0] == INVALID
    assert _call(am=amap, vi_of_node=(), n_nodes=4)[0] == INVALID  # four nodes and no table
    assert _call(am=amap, n_nodes=-1)[0] == INVALID
    assert _call(node_of_file=[0, 4])[0] == INVALID  # a node the table does not have


def test_wrapper_refuses_what_is_no_target(amap):
    with pytest.raises(TypeError):
        host.genome_files_into(["a.fna"], object(), [0, 1, 2, 3], accession_map=amap)
    with pytest.raises(ValueError):
        host.genome_files_into(["a.fna"], object(), [0, 1, 2, 3], accession_map=amap, node_of_file=[0, 1], kind=host.INTO_SIZE)
    with pytest.raises(ga.GsError) as e:  # an object without a handle: the library's NULL check
        host.genome_files_into(["a.fna"], object(), [0, 1, 2, 3], accession_map=amap, kind=host.INTO_SIZE)
    assert e.value.code == INVALID
