"""host.genome_files_into (gs_host_genome_files_into: the genome file loop with the accession map, a table of value indices per node
and one of the four region handles as its target, no callbacks) against the same files driven through gs_host_genome_files_mapped
with ctypes callbacks that apply the same table (tests/genome_into.py).  Per target kind the handle's results -- the build fetch, the
size counts, the update fetch, the quality counts -- are bit-equal, and so are the totals; once with reader blocks that hold the
files whole, once with blocks so small that records straddle them.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import genestrip_amd as ga
import genome_into as gi
from genestrip_amd import host
from progresscheck import check_records, run

pytestmark = pytest.mark.gpu


def _into(paths, node_of_file, amap):
    return lambda target, update: host.genome_files_into(paths, target, gi.VI_OF_NODE, accession_map=amap, node_of_file=node_of_file,
                                                         complete_only=True, update=update)


@pytest.mark.parametrize("block", [65536, 256])
def test_every_target_kind_equals_the_callback_path(block, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", str(block))
    paths, node_of_file = gi.collection(tmp_path)
    amap = gi.accession_map()
    base = gi.base_store(paths, node_of_file, amap)
    assert len(base[0]) > 2000 and set(np.unique(base[1]).tolist()) == {1, 2, 3}
    for kind in gi.KINDS:
        want, want_tot = gi.drive(kind, gi.through_callbacks(paths, node_of_file, amap), base)
        got, got_tot = gi.drive(kind, _into(paths, node_of_file, amap), base)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), kind
        assert got_tot == want_tot, (kind, got_tot, want_tot)
        records, kept, _text, bases, chunks, host_chunks, _line = got_tot[0]
        # 13 records: 3 without a node (no blank, not in the map, dropped by complete_only), 1 whose node has no table entry
        assert (records, kept) == (13, 9) and bases > 2500 and host_chunks >= 1 and chunks > host_chunks, got_tot
        n_chunks = chunks
    # the update pass took LCAs (the shared stretch), the quality counts saw every leaf
    moved = gi.drive("update", _into(paths, node_of_file, amap), base)[0][0]
    assert int(moved[0]) > 0
    if block == 256:  # records straddled blocks: more chunks than with blocks that hold a file whole
        monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
        assert n_chunks > gi.drive("size", _into(paths, node_of_file, amap), base)[1][0][4]
    amap.close()


def test_a_file_given_by_node_needs_no_map(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    paths, _ = gi.collection(tmp_path)
    b = ga.DeviceDbBuilder(gi.K, len(gi.PARENT_VI), gi.PARENT_VI)
    t = host.genome_files_into(paths[3:], b, gi.VI_OF_NODE, node_of_file=[gi.FILE_NODE])
    kmers, vidx = b.finish()
    b.close()
    assert (t.records, t.kept_records) == (2, 2) and len(kmers) > 300 and set(vidx.tolist()) == {int(gi.VI_OF_NODE[gi.FILE_NODE])}


def test_a_failing_add_ends_the_walk_with_its_code(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    paths, node_of_file = gi.collection(tmp_path)
    amap = gi.accession_map()
    s = ga.DeviceDbSizer(gi.K, 2)  # value indices 2 and 3 are no tags of this handle
    with pytest.raises(ga.GsError) as e:
        host.genome_files_into(paths, s, gi.VI_OF_NODE, accession_map=amap, node_of_file=node_of_file)
    assert e.value.code == -1
    s.close()
    amap.close()


def test_cancelling_from_a_control(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "256")
    paths, node_of_file = gi.collection(tmp_path)
    amap = gi.accession_map()
    b = ga.DeviceDbBuilder(gi.K, len(gi.PARENT_VI), gi.PARENT_VI)
    call = lambda: host.genome_files_into(paths, b, gi.VI_OF_NODE, accession_map=amap, node_of_file=node_of_file, complete_only=True)
    _, stop, records = run(call, stop_at=3)  # behind the second chunk of the first file
    assert stop is not None and stop.code == -8
    seen = check_records(records, paths, complete=False)
    assert 0 < stop.totals.records == sum(seen.values()) < 13
    got, stop, records = run(call)
    assert stop is None and got.records == 13 and check_records(records, paths, complete=True) == {0: 5, 1: 4, 2: 2, 3: 2}
    b.close()
    amap.close()
