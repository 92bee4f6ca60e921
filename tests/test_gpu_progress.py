"""Progress and cancellation of the file-level calls on the GPU (include/gshost.h, gs_host_control_*): every input shape of the
match goal -- and the filter, krakencount, genome and extract goals -- with a control attached.  A run that is not stopped gives what
it gives without a control, byte for byte, under records that obey the rules (tests/progresscheck.py); a run stopped at its second
record, in the middle and at its last chunk record returns -8 and leaves a table and per-read outputs that equal the exact reference
(tests/matchcheck.py, tests/krakenlines.py) over the prefix of each file that the last records report; the run is usable afterwards.
Small files, the smallest reader blocks (64 KiB): more than ten chunks each."""
import gzip
import threading
import time

import numpy as np
import pytest

import genestrip_amd as ga
import krakencount as kc
import krakenlines
import matchcheck
from conftest import bgzf
from genestrip_amd import host, synth
from oracle import gs_oracle as orc
from progresscheck import check_records, run

pytestmark = pytest.mark.gpu

N_READS = 3000
C_MAX_CONTIG_READ_NO = 9  # (GS_C_MAX_CONTIG_READ_NO, include/gsgpu.h)


@pytest.fixture(scope="module")
def sdb():
    return synth.SynthDB(k=31, genera=3, species_per_genus=3, genome_len=20000, seed=11)


@pytest.fixture(scope="module")
def store(sdb):
    s = ga.DeviceKMerStore(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)
    yield s
    s.close()


@pytest.fixture(scope="module")
def odb(sdb):
    return orc.DB(31, sdb.kmers, sdb.value_idx, sdb.n_values, sdb.parent_vi)


@pytest.fixture(scope="module")
def reads(sdb):
    seq, off = synth.reads_host(sdb.genomes, N_READS, read_len=150, seed=29)
    seq = seq.copy()
    seq[150 * 40 + 70] = ord("N")
    return [seq[int(off[i]):int(off[i + 1])].tobytes() for i in range(N_READS)]


def _text(reads, shape, first=0):
    if shape == "fasta":
        # (a long comment behind the name: FASTA has no quality lines, and the file shall have more than ten blocks all the same)
        return b"".join(b">r%d s=%d %s\n%s\n%s\n" % (first + i, i % 7, b"c" * 150, s[:80], s[80:]) for i, s in enumerate(reads))
    if shape == "multi-line":
        return b"".join(b"@r%d s=%d\n%s\n%s\n+\n%s\n%s\n" % (first + i, i % 7, s[:70], s[70:], b"F" * 70, b"G" * (len(s) - 70)) for i, s in enumerate(reads))
    return b"".join(b"@r%d s=%d\n%s\n+\n%s\n" % (first + i, i % 7, s, b"F" * len(s)) for i, s in enumerate(reads))


SHAPES = ["four-line", "multi-line", "fasta", "parser", "gz", "bgzf", "two gz"]


def _files(shape, reads, tmp_path, monkeypatch):
    """-> (paths, batch_reads): the input files of a shape, with the settings that cut them into more than ten chunks"""
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    monkeypatch.setenv("GS_HOST_BGZF_TEXT", "65536")
    batch_reads = 0
    if shape in ("four-line", "multi-line", "parser"):
        p = tmp_path / "in.fastq"
        p.write_bytes(_text(reads, "multi-line" if shape == "multi-line" else "four-line"))
        if shape == "parser":
            monkeypatch.setenv("GS_HOST_FAST", "0")
            batch_reads = 900  # (four batches)
        return [str(p)], batch_reads
    if shape == "fasta":
        p = tmp_path / "in.fasta"
        p.write_bytes(_text(reads, "fasta"))
        return [str(p)], 0
    if shape == "bgzf":
        p = tmp_path / "in.fastq.gz"
        p.write_bytes(bgzf(_text(reads, "four-line"), block=20000, level=1))
        return [str(p)], 0
    monkeypatch.setenv("GS_GUNZIP_CHUNK", "4096")
    monkeypatch.setenv("GS_GUNZIP_SLOTS", "5")
    if shape == "gz":
        p = tmp_path / "in.fastq.gz"
        p.write_bytes(gzip.compress(_text(reads, "four-line"), compresslevel=6, mtime=0))
        return [str(p)], 0
    paths = []
    for i, (a, b) in enumerate([(0, 1700), (1700, N_READS)]):
        p = tmp_path / f"part{i}.fastq.gz"
        p.write_bytes(gzip.compress(_text(reads[a:b], "four-line", first=a), compresslevel=6, mtime=0))
        paths.append(str(p))
    return paths, 0


class Reference:
    """the exact reference over a prefix of each file: oracle table and terms, Kraken-style lines, filtered FASTQ"""

    def __init__(self, odb, sdb, paths):
        self.odb, self.sdb, self.parsed = odb, sdb, []
        for p in paths:
            data = matchcheck._file_bytes(p)
            self.parsed.append(orc.parse_fastq(data, fasta=data[:1] == b">", k=31))

    def over(self, counts):
        recs = []
        for p, n in zip(self.parsed, counts):
            assert 0 <= n <= int(p["n_reads"])
            for i in range(n):
                recs.append((bytes(p["desc"][int(p["desc_off"][i]):int(p["desc_off"][i + 1])]),
                             bytes(p["seq"][int(p["seq_off"][i]):int(p["seq_off"][i + 1])])))
        seq = np.frombuffer(b"".join(s for _, s in recs) or b"\0", dtype=np.uint8)
        off = np.cumsum([0] + [len(s) for _, s in recs]).astype(np.uint64)
        o = matchcheck.oracle_batch(self.odb, seq, off)
        lines = b"".join(krakenlines.line(d, len(s), 31, self.odb.segments(s) if len(s) >= 31 else [], int(c), self.sdb.taxids)
                         for (d, s), c in zip(recs, o["class_vi"]))
        flt = b"".join(d + b"\n" + s + b"\n+\n" + b"~" * len(s) + b"\n" for (d, s), f in zip(recs, o["flags"]) if f & orc.F_RETURNED)
        tot = (len(recs), sum(max(0, len(s) - 30) for _, s in recs), sum(len(s) for _, s in recs))
        return o, lines, flt, tot


def _check_state(ref, counts, table, dtable, tot, kraken, filtered, filtered_gz, what):
    o, lines, flt, want_tot = ref.over(counts)
    matchcheck.check_match(o, dict(table=table, dtable=dtable), what)
    assert (tot.reads, tot.kmers, tot.bps) == want_tot, what
    if kraken is not None:
        assert open(kraken, "rb").read() == lines, what
        assert tot.filtered_reads == flt.count(b"\n+\n"), what
    if filtered is not None:
        assert open(filtered, "rb").read() == flt, what
    if filtered_gz is not None:
        raw = open(filtered_gz, "rb").read()
        assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")), what  # a member boundary, then the EOF block
        assert gzip.decompress(raw) == flt, what


@pytest.mark.parametrize("shape", SHAPES)
def test_match_shapes(shape, sdb, store, odb, reads, tmp_path, monkeypatch, request):
    paths, batch_reads = _files(shape, reads, tmp_path, monkeypatch)
    outputs = shape != "two gz"  # (per-read outputs follow the read order: the files would go one after the other)
    ref = Reference(odb, sdb, paths)
    full = [int(p["n_reads"]) for p in ref.parsed]
    assert sum(full) == N_READS

    def outs(tag):
        if not outputs:
            return None, None, None
        return tuple(str(tmp_path / f"{tag}.{x}") for x in ("kraken", "fastq", "fastq.gz"))

    def files_call(tag, gz=False):
        k, f, fz = outs(tag)
        return host.match_files(store, paths, kraken_out_path=k, filtered_path=fz if gz else f, taxids=sdb.taxids, batch_reads=batch_reads)

    # 1. a whole run under a control equals the run without one; the records obey the rules
    t0, d0, tot0 = files_call("plain")
    if outputs:
        files_call("plain", gz=True)
    (t1, d1, tot1), stop, records = run(lambda: files_call("ctl"))
    assert stop is None and np.array_equal(t0, t1)
    # (the double table is summed by atomics in whatever order the waves finish: two runs agree within the bound of that, and each
    # is held to the exact reference below)
    matchcheck.check_dtables_agree(d0, d1, t0[:, 0], "with and without a control")
    assert (tot0.reads, tot0.kmers, tot0.bps, tot0.filtered_reads) == (tot1.reads, tot1.kmers, tot1.bps, tot1.filtered_reads)
    got = check_records(records, paths, complete=True)
    assert [got[f] for f in range(len(paths))] == full and records[-1].total_reads == tot1.reads == N_READS
    chunk_records = [i for i, r in enumerate(records) if r.file_bytes_done > 0 and not r.file_done]
    assert len(chunk_records) > (3 if shape == "parser" else 10), len(chunk_records)
    if shape == "two gz":
        files_of = [r.file for r in records[:-1]]
        assert files_of != sorted(files_of), "the two files interleave their records"
    if outputs:
        run(lambda: files_call("ctl", gz=True))
        for a, b in zip(outs("plain"), outs("ctl")):
            assert open(a, "rb").read() == open(b, "rb").read(), a
        _check_state(ref, full, t1, d1, tot1, *outs("ctl"), "whole run")
    else:
        _check_state(ref, full, t1, d1, tot1, None, None, None, "whole run")

    # 2. + 3. stops at the second record, in the middle and at the last chunk record, into the matcher's own run; then reset and all.
    # Two .gz files: through match_files_into, which reads them side by side (read numbers file << 32 | read, reads_of_file turns the
    # max-contig column into running numbers); every other shape: through match_run, with every per-read output, plain and .gz.
    m = ga.FastqKMerMatcher(store)
    request.addfinalizer(m.close)  # (a store allows one unique-counting run at a time: closed whatever an assertion does)
    side_by_side = shape == "two gz"

    def run_call(tag, gz=False):
        if side_by_side:
            return host.match_files_into(m, paths, list(range(len(paths))))
        k, f, fz = outs(tag)
        return None, host.match_run(m, paths, kraken_out_path=k, filtered_path=fz if gz else f, taxids=sdb.taxids, batch_reads=batch_reads)

    def finish(rof):
        table, dtable = m.finish()
        return (_running(table, rof) if side_by_side else table), dtable

    stops = [2, chunk_records[len(chunk_records) // 2] + 1, chunk_records[-1] + 1]
    for n in stops:
        for gz in ((False, True) if outputs else (False,)):
            got, stop, recs = run(lambda: run_call("stop", gz), stop_at=n)
            assert got is None and stop is not None and stop.code == -8, n
            counts = check_records(recs, paths, complete=False)
            counts = [counts.get(f, 0) for f in range(len(paths))]
            assert recs[-1].total_reads == sum(counts) <= N_READS and (n == stops[-1] or sum(counts) < N_READS)
            if side_by_side:
                assert [int(x) for x in stop.reads_of_file] == counts, n
            table, dtable = finish(counts)
            k, f, fz = outs("stop")
            _check_state(ref, counts, table, dtable, stop.totals, k, None if gz else f, fz if gz else None, f"stop at record {n} (gz {gz})")
            m.reset()
            rof, tot = run_call("again")
            assert not side_by_side or [int(x) for x in rof] == full
            table, dtable = finish(full)
            _check_state(ref, full, table, dtable, tot, *outs("again")[:2], None, f"a whole run after the stop at record {n}")
            m.reset()
    m.close()

    if side_by_side:  # ... and through match_files, whose finish converts the read numbers itself
        n = chunk_records[len(chunk_records) // 2] + 1
        got, stop, recs = run(lambda: files_call("stop"), stop_at=n)
        assert got is None and stop.code == -8
        counts = check_records(recs, paths, complete=False)
        counts = [counts.get(f, 0) for f in range(len(paths))]
        assert 0 < sum(counts) < N_READS
        _check_state(ref, counts, stop.table, stop.dtable, stop.totals, None, None, None, "side by side, stopped")


def _running(table, reads_of_file):
    """the max-contig read numbers of a run that was fed by match_files_into, (file << 32 | read in file), as running numbers over the
    files in order -- what gs_host_match_files does behind its finish"""
    before = np.concatenate([[0], np.cumsum(reads_of_file)]).astype(np.int64)
    t = table.copy()
    x = t[:, C_MAX_CONTIG_READ_NO]
    t[:, C_MAX_CONTIG_READ_NO] = np.where(x >= 0, before[np.maximum(x, 0) >> 32] + (x & 0xFFFFFFFF), x)
    return t


def test_a_file_that_ends_in_the_sweep_of_the_stop(sdb, store, odb, reads, tmp_path, monkeypatch, request):
    """Two .gz files of very unequal length side by side, stopped at the longer file's record that follows the shorter file's last
    block: the short file went through its end (last block, leftover) without a chunk record, in the sweep in which the long one saw
    the stop.  Its last record must say so -- all of its reads are in the table.  The callback holds the long file's record back a
    little once the short file's last chunk record is in, so that the short file's last block is ready in the next sweep."""
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    monkeypatch.setenv("GS_HOST_BGZF_TEXT", "65536")
    monkeypatch.setenv("GS_GUNZIP_CHUNK", "4096")
    monkeypatch.setenv("GS_GUNZIP_SLOTS", "5")
    monkeypatch.setenv("GS_DEVICE_INFLATE", "0")  # (reader blocks: a file's last block ends it without a record)
    n_short = 500
    paths = []
    for i, (a, b) in enumerate([(0, n_short), (n_short, N_READS)]):
        p = tmp_path / f"part{i}.fastq.gz"
        p.write_bytes(gzip.compress(_text(reads[a:b], "four-line", first=a), compresslevel=6, mtime=0))
        paths.append(str(p))
    ref = Reference(odb, sdb, paths)
    _, _, whole = run(lambda: host.match_files(store, paths))
    short_chunks = sum(1 for r in whole if r.file == 0 and r.file_bytes_done > 0 and not r.file_done)
    assert short_chunks >= 1 and sum(1 for r in whole if r.file == 1 and not r.file_done) > 10
    seen = []

    def callback(p):
        seen.append(p)
        mine = sum(1 for r in seen if r.file == 0 and r.file_bytes_done > 0 and not r.file_done)
        if mine < short_chunks or p.file != 1:
            return False
        behind = [r for r in seen[[i for i, r in enumerate(seen) if r.file == 0][-1]:] if r.file == 1]
        if len(behind) == 1:
            time.sleep(0.05)  # the short file's last block is inflated meanwhile
            return False
        return True

    m = ga.FastqKMerMatcher(store)
    request.addfinalizer(m.close)
    for call in ("into", "files"):
        seen.clear()
        with host.Control(callback):
            with pytest.raises(host.Cancelled) as e:
                host.match_files_into(m, paths, [0, 1]) if call == "into" else host.match_files(store, paths)
        counts = check_records(seen, paths, complete=False)
        counts = [counts.get(0, 0), counts.get(1, 0)]
        assert counts[0] == n_short and 0 < counts[1] < N_READS - n_short, (call, counts)
        assert any(r.file == 0 and r.file_done for r in seen), "the short file's last record"
        if call == "into":
            assert [int(x) for x in e.value.reads_of_file] == counts
            table, dtable = m.finish()
            _check_state(ref, counts, _running(table, counts), dtable, e.value.totals, None, None, None, "match_files_into: a file ended in the sweep of the stop")
            m.close()  # (match_files begins a run of its own on the store)
        else:
            _check_state(ref, counts, e.value.table, e.value.dtable, e.value.totals, None, None, None, "match_files: a file ended in the sweep of the stop")


def test_match_files_stopped_fills_its_table(sdb, store, odb, reads, tmp_path, monkeypatch):
    paths, _ = _files("four-line", reads, tmp_path, monkeypatch)
    ref = Reference(odb, sdb, paths)
    k, f, fz = (str(tmp_path / x) for x in ("o.kraken", "o.fastq", "o.fastq.gz"))
    for flt in (f, fz):
        got, stop, recs = run(lambda: host.match_files(store, paths, kraken_out_path=k, filtered_path=flt, taxids=sdb.taxids), stop_at=6)
        assert got is None and stop.code == -8
        n = recs[-1].file_reads
        assert 0 < n < N_READS
        _check_state(ref, [n], stop.table, stop.dtable, stop.totals, k, f if flt == f else None, fz if flt == fz else None, "match_files, stopped")


def test_cancel_from_a_second_thread(sdb, store, odb, reads, tmp_path, monkeypatch):
    paths, _ = _files("four-line", reads, tmp_path, monkeypatch)
    ref = Reference(odb, sdb, paths)
    k, f = str(tmp_path / "o.kraken"), str(tmp_path / "o.fastq.gz")
    seen = []

    def slow(p):  # (keeps the call running while the other thread gets to its cancel)
        seen.append(p)
        time.sleep(0.02)
        return False

    with host.Control(slow) as ctl:
        def canceller():
            while ctl.snapshot()[0].file_bytes_done == 0:
                time.sleep(0.001)
            ctl.cancel()
        t = threading.Thread(target=canceller)
        t.start()
        with pytest.raises(host.Cancelled) as e:
            host.match_files(store, paths, kraken_out_path=k, filtered_path=f, taxids=sdb.taxids)
        t.join()
        last, flag = ctl.snapshot()
    assert flag and e.value.code == -8
    counts = check_records(seen, paths, complete=False)
    assert last.file_reads == counts[0] == e.value.totals.reads and 0 < counts[0] < N_READS
    _check_state(ref, [counts[0]], e.value.table, e.value.dtable, e.value.totals, k, None, f, "cancel from a second thread")


def _prefix_records(data, n):
    return b"".join(data.splitlines(keepends=True)[:4 * n])


@pytest.mark.parametrize("gz_out", [False, True])
def test_filter_files(gz_out, sdb, reads, tmp_path, monkeypatch):
    paths, _ = _files("four-line", reads, tmp_path, monkeypatch)
    data = open(paths[0], "rb").read()
    keys = sdb.kmers[np.isin(sdb.value_idx, sdb.species_vi[:4])]
    ob = orc.Bloom(orc.BLOOM_XOR, len(keys), 1e-8)
    ob.put_many(keys)
    gb = ga.DeviceBloomFilter(ga.BLOOM_XOR, ob.bits, ob.hash_factors, ob.words)
    ext = ".fastq.gz" if gz_out else ".fastq"

    def call(tag):
        return host.filter_files(gb, 31, paths, filtered_path=str(tmp_path / (tag + ".acc" + ext)), rest_path=str(tmp_path / (tag + ".rest" + ext)))

    def out(tag, which):
        raw = open(str(tmp_path / (tag + "." + which + ext)), "rb").read()
        return gzip.decompress(raw) if gz_out else raw

    def want(n):
        p = orc.parse_fastq(_prefix_records(data, n), k=31)
        acc = ob.filter_batch(31, 1, 0.2, p["seq"], p["seq_off"]) if n else np.zeros(0, bool)
        a, r = bytearray(), bytearray()
        for i in range(n):
            d = bytes(p["desc"][int(p["desc_off"][i]):int(p["desc_off"][i + 1])])
            s = bytes(p["seq"][int(p["seq_off"][i]):int(p["seq_off"][i + 1])])
            (a if acc[i] else r).extend(d + b"\n" + s + b"\n+\n" + b"~" * len(s) + b"\n")
        return bytes(a), bytes(r), int(acc.sum())

    tot0 = call("plain")
    tot1, stop, records = run(lambda: call("ctl"))
    assert stop is None and (tot0.reads, tot0.filtered_reads) == (tot1.reads, tot1.filtered_reads) == (N_READS, want(N_READS)[2])
    assert check_records(records, paths, complete=True)[0] == N_READS and len(records) > 12
    for which in ("acc", "rest"):
        assert open(str(tmp_path / ("plain." + which + ext)), "rb").read() == open(str(tmp_path / ("ctl." + which + ext)), "rb").read()
    assert (out("ctl", "acc"), out("ctl", "rest")) == want(N_READS)[:2]
    for n in (2, len(records) // 2, len(records) - 2):
        got, stop, recs = run(lambda: call("stop"), stop_at=n)
        assert got is None and stop.code == -8
        k = check_records(recs, paths, complete=False)[0]
        a, r, n_acc = want(k)
        assert (out("stop", "acc"), out("stop", "rest")) == (a, r), n
        assert (stop.totals.reads, stop.totals.filtered_reads) == (k, n_acc) and k <= N_READS
    gb.close()


def test_extract_on_the_device(reads, tmp_path, monkeypatch):
    import streamgoals as sg
    paths, _ = _files("four-line", reads, tmp_path, monkeypatch)
    data = open(paths[0], "rb").read()
    dst = tmp_path / "out.fastq.gz"
    call = lambda: host.extract_files(b"r1", paths, dst, k=31)
    tot0 = call()
    raw0 = dst.read_bytes()
    tot1, stop, records = run(call)
    assert stop is None and dst.read_bytes() == raw0 and gzip.decompress(raw0) == sg.extract(data, b"r1")[0]
    assert check_records(records, paths, complete=True)[0] == N_READS == tot1.reads and tot1.filtered_reads == tot0.filtered_reads
    for n in (2, len(records) // 2, len(records) - 2):
        got, stop, recs = run(call, stop_at=n)
        k = check_records(recs, paths, complete=False)[0]
        want, n_sel = sg.extract(_prefix_records(data, k), b"r1")
        assert gzip.decompress(dst.read_bytes()) == want and (stop.totals.reads, stop.totals.filtered_reads) == (k, n_sel), n


def test_kraken_count_files(tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    lines = [b"C\tr%d\t%d\t150\t%d:%d 0:%d A:1 %d:3\n" % (i, 100 + i % 7, 100 + i % 7, 20 + i % 50, i % 9, 200 + i % 3) for i in range(24000)]
    data = b"".join(lines)
    p = tmp_path / "k.out"
    p.write_bytes(data)
    paths = [str(p)]
    call = lambda: host.kraken_count_files(paths)
    rows0, tot0 = call()
    (rows1, tot1), stop, records = run(call)
    assert stop is None and rows1 == rows0 == kc.count(data)[0] and tot1["lines"] == 24000 and tot1["device_chunks"] > 10
    assert check_records(records, paths, complete=True)[0] == 24000
    for n in (2, len(records) // 2, len(records) - 2):
        got, stop, recs = run(call, stop_at=n)
        k = check_records(recs, paths, complete=False)[0]
        assert got is None and stop.code == -8 and k <= 24000
        assert stop.rows == kc.count(b"".join(lines[:k]))[0] and stop.totals["lines"] == k, n


def test_genome_files(sdb, tmp_path, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", "65536")
    genomes = [sdb.genomes[i % len(sdb.genomes)].tobytes()[:6000 + 500 * (i % 5)] for i in range(40)]
    data = b"".join(b">g%d x\n" % i + b"".join(g[j:j + 70] + b"\n" for j in range(0, len(g), 70)) for i, g in enumerate(genomes))
    p = tmp_path / "g.fasta"
    p.write_bytes(data)
    paths = [str(p)]
    got = []

    def resolve(file, first, headers):
        assert [h.split()[0] for h in headers] == [b">g%d" % (first + i) for i in range(len(headers))]
        return [first + i for i in range(len(headers))]

    def sink(seq, off, vi):
        s = seq.numpy().tobytes() if hasattr(seq, "numpy") else bytes(seq)
        o = off.numpy() if hasattr(off, "numpy") else np.asarray(off)
        got.extend((int(v), s[int(o[i]):int(o[i + 1])]) for i, v in enumerate(vi))
        return 0

    call = lambda: host.genome_files(paths, resolve, sink)
    tot, stop, records = run(call)
    assert stop is None and tot.records == 40 and got == list(enumerate(genomes))
    assert check_records(records, paths, complete=True)[0] == 40 and len(records) > 5
    for n in (2, len(records) // 2, len(records) - 2):
        got.clear()
        res, stop, recs = run(call, stop_at=n)
        k = check_records(recs, paths, complete=False)[0]
        assert res is None and stop.code == -8 and k <= 40
        assert got == list(enumerate(genomes))[:k] and stop.totals.records == k, n
