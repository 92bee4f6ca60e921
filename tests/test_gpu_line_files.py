"""What the four line-catalog goals share in their file loops (gs_host.cpp: accmap, asmsum, taxtree, krakencount), held to one set
of cases: files of lines cut into chunks of whole lines for the device; a chunk the device refuses goes through the exact host parser
at its place in the input order; a line longer than a reader block, or an unterminated tail, sends the rest of the file through that
parser.  Every case compares the device run with the GS_HOST_FAST=0 run of the same files and with the goal's plain-Python
restatement (tests/accmap.py, asmsum.py, taxtree.py, krakencount.py).  Files of a few tens of KB at reader blocks of 4096 bytes: ten
or so chunks each.  Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import asmsum
import genestrip_amd as ga
import krakencount as kc
import taxtree
from accmap_cases import CFG, KNOWN, catalog
from accmap_cases import L as AL
from asmsum_cases import FTP, rec
from genestrip_amd import host
from krakencount_cases import line as kline
from krakencount_cases import long_line, random_text
from progresscheck import check_records, run
from taxtree_cases import N, random_dump
from test_gpu_accmap_files import _expect, _map_of
from test_gpu_asmsum_files import _as_tuples
from test_gpu_krakencount_files import _totals

pytestmark = pytest.mark.gpu

BLOCK = 4096
GOALS = ["accmap", "asmsum", "taxtree", "krakencount"]
AS_KNOWN = sorted({7, 562, 9606, 10090} | {1000 + 13 * i for i in range(40)})
TREE_KEYS = ("taxids", "parent", "depth", "position", "subtree", "rank")
# a line of this many bytes holds a whole reader block without a newline, wherever it starts: the cutter gives the file up there
LONG = 3 * BLOCK


def _lines(data):
    return data.splitlines(keepends=True)


def _at(lines, num, den):
    """the lines in front of and behind about num/den of the text"""
    k = len(lines) * num // den
    return b"".join(lines[:k]), b"".join(lines[k:])


class Goal:
    """one goal: its regular text, its lines of each kind, its call and its restatement.  A result is a value to compare with ==;
    chunks = (device_chunks, host_chunks); lines = the lines of all files"""

    def __init__(self, name):
        self.name = name

    # ---- texts
    def regular(self, seed):
        if self.name == "accmap":
            return catalog(600, seed)
        if self.name == "asmsum":
            return asmsum.summary(110, AS_KNOWN, seed=seed)
        if self.name == "taxtree":
            return random_dump(1400, seed=seed, max_id=90000)
        return random_text(np.random.default_rng(seed), 36000)

    def refused_line(self):
        """one line outside the device's grammar that the host parser takes"""
        return {"accmap": b"7\tx\tNC_9\tbacteria\tREVIEWED\n",  # four tabs
                "asmsum": rec(taxid=b"7") + b"\r\n",
                "taxtree": b"77\t|\n",  # one bar
                "krakencount": kline(b"7:5 007:2", cls=b"007")}[self.name]

    def long_line(self):
        """one line of more than LONG bytes in the file that every parser takes"""
        if self.name == "accmap":  # (a line of the text holds at most 2048 bytes; NUL bytes are dropped in front of the parser)
            return b"562\tx\tNC_777777.1\tbact" + b"\0" * LONG + b"eria\tREVIEWED\t1\n"
        if self.name == "asmsum":
            return rec(organism=b"E" * LONG) + b"\n"
        if self.name == "taxtree":  # (the parser cuts a line at 4096 bytes; NUL bytes are dropped in front of it here as well)
            return b"89999\t|\t1\t|\tspe" + b"\0" * LONG + b"cies\t|\n"
        return long_line(LONG)

    def bad_line(self):
        """one line that fails the call, and the library's words for it (as the library gave them before the loops were folded)"""
        return {"accmap": (AL("7", "NC_1", name="n" * 2100), -1),
                "asmsum": (rec(ftp=b"") + b"\n", -1),
                "taxtree": (b"1\t||\n", -1),  # (a names line of the root whose name has a negative length)
                "krakencount": (kline(b"9:5x"), -1)}[self.name]

    # ---- files: taxtree takes two, the nodes and the names; `text` is the nodes text there
    def names_of(self, nodes):
        ref = taxtree.Tree(taxtree.nodes_slots(nodes))
        return b"".join(N(int(t), f"n{t}", "scientific name" if t % 2 else "synonym") for t in ref.taxids) + N(1, "a synonym of the root")

    def write(self, tmp_path, texts):
        paths = []
        for i, t in enumerate(texts):
            paths.append(str(tmp_path / f"{self.name}{i}.txt"))
            with open(paths[-1], "wb") as f:
                f.write(t)
        return paths

    # ---- the call: -> (result, chunks, lines)
    def call(self, paths):
        if self.name == "accmap":
            m, tot = host.accmap_files(paths, KNOWN, **CFG)
            got = _map_of(m, tot)
            m.close()
            return got, (tot["device_chunks"], tot["host_chunks"]), tot["lines"]
        if self.name == "asmsum":
            picks, total, tot = host.assembly_summary_files(paths, AS_KNOWN, max_per_taxid=0)
            return (_as_tuples(picks), total, tot["kept"]), (tot["device_chunks"], tot["host_chunks"]), tot["lines"]
        if self.name == "taxtree":
            t, rep = host.taxtree_files(*paths)
            a = t.arrays()
            got = tuple(a[k].tolist() for k in TREE_KEYS), t.names(), tuple(rep[k] for k in ("nodes", "reached", "duplicates", "nodes_lines", "names_lines"))
            t.close()
            return got, (rep["device_chunks"], rep["host_chunks"]), rep["nodes_lines"] + rep["names_lines"]
        rows, tot = host.kraken_count_files(paths)
        return (rows, _totals(tot)), (tot["device_chunks"], tot["host_chunks"]), tot["lines"]

    def stopped_lines(self, stop):
        """the lines a stopped call says it has worked off"""
        if self.name == "taxtree":
            return stop.report["nodes_lines"] + stop.report["names_lines"]
        return stop.totals["lines"]

    # ---- the restatement: -> the result that call() gives, without what only the library knows
    def restated(self, texts):
        if self.name == "accmap":
            return _expect(texts)
        if self.name == "asmsum":
            c = asmsum.cfg(AS_KNOWN)
            entries, counted, first = [], 0, 0
            for t in texts:
                e, n, short, skipped = asmsum.relevant_entries(t, c, first_line=first)
                entries, counted, first = entries + e, counted + n, first + n + short + skipped
            return asmsum.cap(entries, 0), counted, len(entries)
        if self.name == "taxtree":
            ref = taxtree.Tree(taxtree.nodes_slots(texts[0]))
            if len(texts) > 1:
                ref.read_names(texts[1])
            return tuple(getattr(ref, k).tolist() for k in TREE_KEYS), ref.names
        rows = {}
        tot = [0, 0, 0, 0]
        for t in texts:
            r, tt = kc.count(t)
            for k, *v in r:
                rows[k] = [x + y for x, y in zip(rows.get(k, [0, 0, 0]), v)]
            tot = [x + y for x, y in zip(tot, tt.values())]
        return [(k, *rows[k]) for k in sorted(rows)], tuple(tot)

    def check_restated(self, got, texts):
        want = self.restated(texts)
        assert got[:len(want)] == want, (self.name, [g == w for g, w in zip(got, want)])


@pytest.fixture(params=GOALS)
def goal(request, monkeypatch):
    monkeypatch.setenv("GS_HOST_BLOCK_BYTES", str(BLOCK))
    return Goal(request.param)


def _both_ways(goal, paths, monkeypatch):
    """the call on the device and under GS_HOST_FAST=0 -> (result, chunks, lines) of the device run; the results are equal"""
    dev = goal.call(paths)
    monkeypatch.setenv("GS_HOST_FAST", "0")
    hst = goal.call(paths)
    monkeypatch.delenv("GS_HOST_FAST")
    print(goal.name, "device", dev[1:], "host only", hst[1:])
    assert hst[1][0] == 0, "GS_HOST_FAST=0 sent a chunk to the device"
    assert dev[0] == hst[0] and dev[2] == hst[2], (goal.name, dev[1:], hst[1:])
    return dev


def _texts(goal, first):
    """the files of a one-stream case: taxtree takes its names file with the nodes"""
    return [first, goal.names_of(first)] if goal.name == "taxtree" else [first]


def test_a_refused_chunk_in_the_middle(goal, tmp_path, monkeypatch):
    head, rest = _at(_lines(goal.regular(11)), 1, 2)
    text = head + goal.refused_line() + rest
    texts = _texts(goal, text)
    got, (device_chunks, host_chunks), _ = _both_ways(goal, goal.write(tmp_path, texts), monkeypatch)
    goal.check_restated(got, texts)
    assert host_chunks >= 1 and device_chunks >= 2
    if goal.name == "asmsum":  # the entries behind the refused chunk carry stream line numbers
        odd = len(asmsum.lines_of(head))
        assert (0, b"7", b"562", FTP, 1, False, odd) in got[0] and max(e[6] for e in got[0]) > odd + 20


def test_a_line_longer_than_the_reader_block(goal, tmp_path, monkeypatch):
    head, rest = _at(_lines(goal.regular(13)), 1, 3)
    text = head + goal.long_line() + rest
    texts = _texts(goal, text)
    got, (device_chunks, host_chunks), _ = _both_ways(goal, goal.write(tmp_path, texts), monkeypatch)
    goal.check_restated(got, texts)
    assert device_chunks >= 1 and host_chunks >= 1


def test_no_final_newline(goal, tmp_path, monkeypatch):
    text = goal.regular(17)[:-1]
    texts = _texts(goal, text)
    if goal.name == "taxtree":
        texts[1] = texts[1][:-1]
    got, (device_chunks, host_chunks), _ = _both_ways(goal, goal.write(tmp_path, texts), monkeypatch)
    goal.check_restated(got, texts)
    assert device_chunks >= 2 and host_chunks >= 1  # (the tail: a memory range)


# the library's words behind "<path>: " for bad_line() as line n of its file
ERRORS = {
    "accmap": "line {n}: buffer is too small for a line in the accession catalog file",
    "asmsum": "line {n}: a kept entry has an empty ftp path",
    "taxtree": "names line {n}: a name of negative length (StringIndexOutOfBoundsException)",
    "krakencount": "line {n}: non-digit in a number",
}


def test_two_files_and_a_format_error_in_the_second(goal, tmp_path, monkeypatch):
    """the message names the second file and the line's number in that file, whichever way the line's chunk went"""
    first = goal.regular(19)
    bad, code = goal.bad_line()
    if goal.name == "taxtree":
        names = _lines(goal.names_of(first))
        head, rest = _at(names, 2, 5)
    else:
        head, rest = _at(_lines(goal.regular(23)), 2, 5)
    texts = [first, head + bad + rest]
    paths = goal.write(tmp_path, texts)
    n = head.count(b"\n") + 1
    assert first.count(b"\n") > 100  # (the line's number in the stream is another)
    said = []
    for fast in ("1", "0"):
        monkeypatch.setenv("GS_HOST_FAST", fast)
        with pytest.raises(ga.GsError) as e:
            goal.call(paths)
        print(goal.name, "GS_HOST_FAST=" + fast, e.value.code, str(e.value))
        assert e.value.code == code and paths[1] in str(e.value) and paths[0] not in str(e.value)
        assert f"line {n}: " in str(e.value)
        said.append(str(e.value).split(paths[1] + ": ", 1)[1])
    assert said == [ERRORS[goal.name].format(n=n)] * 2


def test_cancellation_on_the_second_chunk(goal, tmp_path, monkeypatch):
    """stopped behind the second chunk of the first file: the last record is the record of the stop for file 0, and its lines are the
    lines of the text in front of where the loop stands -- as in every record of the device run; the host-only run ends on the same
    lines per file"""
    texts = _texts(goal, goal.regular(29))
    paths = goal.write(tmp_path, texts)
    call = lambda: goal.call(paths)
    (_, (device_chunks, _), lines), stop, records = run(call)
    assert stop is None and device_chunks >= 8
    last = check_records(records, paths, complete=True)
    assert sum(last.values()) == lines == sum(t.count(b"\n") for t in texts)
    for r in records:
        assert r.file_reads == texts[r.file][:r.file_bytes_done].count(b"\n"), r
    monkeypatch.setenv("GS_HOST_FAST", "0")
    (_, _, lines_host), stop, records_host = run(call)
    monkeypatch.delenv("GS_HOST_FAST")
    assert stop is None and lines_host == lines and check_records(records_host, paths, complete=True) == last
    got, stop, recs = run(call, stop_at=3)  # the first record of file 0, its first chunk, its second chunk
    assert got is None and stop is not None and stop.code == -8
    k = check_records(recs, paths, complete=False)[0]
    assert len(recs) == 4 and recs[-1].file == 0 and recs[-1].file_done == 0 and recs[-1].files_done == 0
    assert [r.file_reads for r in recs] == [r.file_reads for r in records[:3]] + [k] and recs[-1].file_reads == recs[-2].file_reads
    assert 0 < k < texts[0].count(b"\n") and k == texts[0][:recs[-1].file_bytes_done].count(b"\n")
    assert goal.stopped_lines(stop) == k
