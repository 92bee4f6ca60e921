"""What tests/test_gpu_genome_files_into.py and tests/test_gpu_jni_dbchain.py share: a genome collection of a few kilobytes that
holds every case the file loop treats differently, a tree of four nodes with its table of value indices, and the drivers that send
the collection into each of the four region handles -- once through the callbacks of gs_host_genome_files_mapped (the yardstick),
once through whatever callback-free call the test is about."""
import gzip

import numpy as np

import genestrip_amd as ga
from conftest import bgzf
from genestrip_amd import host

K = 31
KNOWN = [7, 562, 9606, 10090]                        # nodes 0 .. 3
PARENT_VI = np.array([-1, 0, 0, 1], dtype=np.int32)  # value indices 0 .. 3
VI_OF_NODE = np.array([1, 2, -1, 3], dtype=np.int32)  # node 2: in the map, not in the table
MAP_ENTRIES = [(b"NC_000001.1", 0), (b"NZ_AB0002.2", 1), (b"NC_000003.1", 2), (b"NC_000004.7", 3), (b"WP_000005.1", 1), (b"NC_000006.1", 3)]
FILE_NODE = 1                                        # the node of every record of the fourth file
KINDS = ("size", "build", "update", "quality")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def _record(header, body, eol=b"\n", width=60):
    return header + eol + b"".join(body[j:j + width] + eol for j in range(0, len(body), width))


def collection(tmp_path):
    """-> (paths, node_of_file): plain, single-member gzip, BGZF, and a plain file whose node node_of_file gives.  `shared` lies in
    records of value indices 1 and 3 and of 2 and 3, so an update pass has LCAs to take."""
    rng = np.random.default_rng(4711)
    shared = _bases(rng, 150)
    a = (_record(b">NC_000001.1 Some species, complete genome", _bases(rng, 400) + shared) +
         _record(b">NC_000004.7", _bases(rng, 300)) +                                        # a header without a blank: no node
         _record(b">NC_404404.1 not in the map", _bases(rng, 200)) +                         # an accession the map lacks
         _record(b">NC_000003.1 its node has no table entry", _bases(rng, 250)) +            # table entry -1
         _record(b">NC_000004.7 lower case and N", shared + _bases(rng, 120).lower() + b"NNNNNnn" + _bases(rng, 180)))
    b = (_record(b">NZ_AB0002.2 CRLF lines", _bases(rng, 330) + shared, eol=b"\r\n") +
         b">NC_000006.1 no data lines\n" +                                                     # a record without data lines
         _record(b">WP_000005.1 in the map, dropped by complete_only", _bases(rng, 200)) +
         _record(b">NC_000006.1 with a NUL", _bases(rng, 90) + b"\0" + _bases(rng, 140)))     # -> the host parser
    c = (_record(b">NC_000004.7 third file", _bases(rng, 500)) +
         _record(b">NC_000001.1 ends without a newline", _bases(rng, 333))[:-1])             # a last line without newline
    d = (_record(b">anything at all", _bases(rng, 280)) + b"\n" +
         _record(b">NC_000004.7 the map is not asked", shared + _bases(rng, 100)))
    paths = [tmp_path / "a.fna", tmp_path / "b.fna.gz", tmp_path / "c.fna.gz", tmp_path / "d.fasta"]
    paths[0].write_bytes(a)
    paths[1].write_bytes(gzip.compress(b, 6))
    paths[2].write_bytes(bgzf(c, block=300))
    paths[3].write_bytes(d)
    assert sum(len(x) for x in (a, b, c, d)) < 8192
    return [str(p) for p in paths], np.array([-1, -1, -1, FILE_NODE], dtype=np.int32)


def accession_map(device=0):
    m = ga.DeviceAccessionMap(KNOWN, ["bacteria"], ["REVIEWED"], device=device)
    m.append([k for k, _ in MAP_ENTRIES], [n for _, n in MAP_ENTRIES])
    m.finish()
    return m


def base_store(paths, node_of_file, amap):
    """the arrays of a store built (without update passes) from the collection through the callbacks: what update and quality start from"""
    b = ga.DeviceDbBuilder(K, len(PARENT_VI), PARENT_VI)
    host.genome_files_mapped(paths, amap, _table_resolver(node_of_file), lambda s, o, v: b.add(s, o, v), complete_only=True)
    out = b.finish()
    b.close()
    return out


def _table_resolver(node_of_file):
    def resolve(file, _first, node):
        if node_of_file[file] >= 0:
            node = np.full(len(node), node_of_file[file], dtype=np.int32)
        return np.where(node >= 0, VI_OF_NODE[np.maximum(node, 0)], -1).astype(np.int32)
    return resolve


def through_callbacks(paths, node_of_file, amap):
    """walk(target, update) for drive(): gs_host_genome_files_mapped with ctypes callbacks that apply the same table"""
    def walk(target, update):
        add = (lambda s, o, v: target.add(s, o, v, update=update)) if isinstance(target, ga.DeviceDbBuilder) else target.add
        return host.genome_files_mapped(paths, amap, _table_resolver(node_of_file), add, complete_only=True)
    return walk


def totals_of(t):
    return (t.records, t.kept_records, t.text_bytes, t.kept_bases, t.chunks, t.host_chunks, t.max_line_bytes)


def drive(kind, walk, base):
    """the collection into a fresh handle of `kind` through walk(target, update) -> (results as a list of arrays, totals per pass)"""
    if kind == "size":
        t = ga.DeviceDbSizer(K, len(PARENT_VI), keep_keys=True, radix_bits=16)
        tot = [walk(t, False)]
        c, per_value, hist = t.counts()
        n, buckets = t.distinct()
        res = [np.array([c.total, c.dust, c.included, n]), per_value, hist, buckets]
    elif kind == "build":
        t = ga.DeviceDbBuilder(K, len(PARENT_VI), PARENT_VI)
        tot = [walk(t, False), walk(t, True)]
        res = list(t.finish())
    elif kind == "update":
        t = ga.DeviceDbUpdater.from_arrays(K, base[0], base[1], len(PARENT_VI), PARENT_VI)
        tot = [walk(t, False)]
        moved = t.finish()
        res = [np.array([moved])] + list(t.fetch())
    else:
        store = ga.DeviceKMerStore(K, base[0], base[1], len(PARENT_VI), PARENT_VI)
        t = ga.DeviceDbQuality(store)
        tot = [walk(t, False)]
        res = list(t.finish())
        t.close()
        store.close()
        return res, [totals_of(x) for x in tot]
    t.close()
    return res, [totals_of(x) for x in tot]
