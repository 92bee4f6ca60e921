"""Rates of the accession map goals.

    python tools/accmap_rate.py [lines]

A synthetic RefSeq catalog of `lines` lines (default 5 000 000) whose field lengths copy a real catalog line
(`9606\\tHomo sapiens\\tNC_000001.11\\tcomplete|vertebrate_mammalian\\tVALIDATED\\t248956422`): three lines in four are protein records,
which fail at the prefix; the lines are drawn from a pool of 65 536, so the map holds repeated accessions.
* per pass, between events (gs_accmap_kernel_time), the chunk resident in device memory, five timed turns after one untimed, the
  fastest and the spread: the count pass alone (a map without a tree puts nothing, so no write pass runs), count + write, the finish,
  and a lookup of 1 000 000 header lines in device memory;
* beside them, on the same bytes, the two yardsticks already in the tree: the kernels of gs_krakencount and the four-line text stage
  of gs_reads (the chunk is refused by both: only their scans are timed);
* the accmap goal end to end from a plain and a .gz file (gs_host_accmap_files), device path against GS_HOST_FAST=0 (the line-by-line
  parser), by turns, on the host clock."""
import ctypes as C
import gzip
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host  # noqa: E402

CATEGORIES = ["bacteria", "archaea", "viral"]
STATUSES = ["REVIEWED", "VALIDATED", "PROVISIONAL"]


def text(n):
    rng = np.random.default_rng(11)
    known = np.unique(rng.integers(2, 3000000, 20000)).astype(np.int32)
    cats = ["complete|bacteria", "bacteria", "complete|vertebrate_mammalian", "vertebrate_other", "viral", "plant|complete", "archaea", "fungi"]
    stats = ["REVIEWED", "VALIDATED", "PROVISIONAL", "PREDICTED", "MODEL", "INFERRED", "na"]
    names = ["Homo sapiens", "Escherichia coli str. K-12 substr. MG1655", "Mus musculus", "Klebsiella pneumoniae", "Bacillus subtilis subsp. subtilis"]
    pool = []
    for i in range(65536):
        u = rng.random()
        prefix = ["WP_", "XP_", "NP_", "YP_"][i & 3] if u < 0.75 else ["NC_", "NZ_", "NW_", "NT_", "XM_", "NM_", "XR_", "AC_"][int(rng.integers(0, 8))]
        taxid = int(known[int(rng.integers(0, len(known)))]) if rng.random() < 0.8 else int(rng.integers(3000000, 4000000))
        acc = prefix + ("%09d.%d" % (i, 1 + i % 3) if prefix[1] == "P" or prefix[0] == "X" else "%06d.%d" % (i % 1000000, 1 + i % 12))
        pool.append(b"%d\t%s\t%s\t%s\t%s\t%d\n" % (taxid, names[i % len(names)].encode(), acc.encode(), cats[int(rng.integers(0, len(cats)))].encode(),
                                                     stats[int(rng.integers(0, len(stats)))].encode(), int(rng.integers(100, 250000000))))
    return b"".join(pool[i] for i in rng.integers(0, len(pool), n)), known


def turns(run, label, mb=None):
    """one untimed and five timed turns of run() -> milliseconds per turn; prints the fastest and the spread"""
    run()
    ms = sorted(run() for _ in range(5))
    rate = f" = {mb / ms[0]:.1f} GB/s of text" if mb else ""
    print(f"{label}: {ms[0]:.3f} ms fastest of 5 (slowest {ms[-1]:.3f}){rate}")
    return ms[0]


def main():
    import torch

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 5000000
    data, known = text(n)
    mb = len(data) / 1e6
    print(f"{n} lines, {mb:.1f} MB")
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    state = {}

    def timed(m, what):
        before = m.kernel_time(True)[1]
        what()
        return m.kernel_time(True)[1] - before

    def count_only():
        m = ga.DeviceAccessionMap([], CATEGORIES, STATUSES, "ALL")
        ms = timed(m, lambda: state.update(rep=m.submit(dev, last=True)))
        m.close()
        return ms

    def count_and_write():
        if state.get("map"):
            state["map"].close()
        m = state["map"] = ga.DeviceAccessionMap(known, CATEGORIES, STATUSES, "ALL", reserve_entries=n // 8)
        return timed(m, lambda: state.update(rep=m.submit(dev, last=True)))

    def finish():
        count_and_write()
        return timed(state["map"], lambda: state.update(info=state["map"].finish()))

    t_count = turns(count_only, "count pass (tiles, scan, count)", mb)
    assert state["rep"]["refused"] == 0 and state["rep"]["put"] == 0
    t_both = turns(count_and_write, "count + write pass", mb)
    rep = state["rep"]
    print(f"  {rep['lines']} lines, {rep['passing']} pass, {rep['put']} put; the write pass alone: {t_both - t_count:.3f} ms")
    turns(finish, "finish (four word sorts, permute, duplicates)")
    print("  entries %d, passing %d, duplicates %d, conflicts %d" % state["info"])
    m = state["map"]
    slots = ga.slot_accessions(m.fetch()[0][:: max(m.n_entries // 50000, 1)])
    rng = np.random.default_rng(3)
    headers = [b">" + (slots[int(rng.integers(0, len(slots)))] if i % 4 else b"NC_%06d.1" % i) + b" Escherichia coli chromosome, complete genome" for i in range(1000000)]
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(h) for h in headers])]).astype(np.int64)).to("cuda:0")
    flat = torch.frombuffer(bytearray(b"".join(headers)), dtype=torch.uint8).to("cuda:0")
    turns(lambda: timed(m, lambda: state.update(nodes=m.lookup(flat, off, complete_only=True))), "lookup of 1 000 000 header lines")
    print(f"  {int((state['nodes'] >= 0).sum())} of them found")
    m.close()

    # the yardsticks on the same bytes
    kc = ga.KrakenCounter(0)

    def kraken():
        before = kc.kernel_time(True)[1]
        assert kc.chunk(kc.submit(dev))["refused"] == 1
        return kc.kernel_time(True)[1] - before
    turns(kraken, "yardstick, gs_krakencount kernels (refused: count, scans, check)", mb)
    kc.close()
    reads = ga.DeviceReads(k=31)
    L = ga.lib()
    acc = torch.zeros(max(n // 4, 1), dtype=torch.uint8, device="cuda:0")
    key = np.frombuffer(b"x", dtype=np.uint8)
    nl = n & ~3
    cut = len(data) if nl == n else int(np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)[nl - 1]) + 1
    reads.kernel_time(True)

    def four_line():
        before = reads.phase_times()["select"][1]
        L.gs_reads_select_text(reads.h, 31, C.c_void_p(dev.data_ptr()), cut, nl, ga.MEM_DEVICE, key.ctypes.data_as(C.c_void_p), 1, C.c_void_p(acc.data_ptr()), None, None)
        L.gs_reads_sync(reads.h)
        reads.text_reset(True)
        return reads.phase_times()["select"][1] - before
    turns(four_line, "yardstick, gs_reads four-line text stage (refused)", cut / 1e6)
    reads.close()

    # end to end: gs_host_accmap_files from a plain and a .gz file, the device path by turns with GS_HOST_FAST=0 (the line-by-line
    # parser into a host-only map), on the host clock
    tmp = tempfile.mkdtemp()
    plain, gz = os.path.join(tmp, "c.catalog"), os.path.join(tmp, "c.catalog.gz")
    open(plain, "wb").write(data)
    open(gz, "wb").write(gzip.compress(data, 1))
    for name, path in (("plain", plain), (".gz", gz)):
        t = {"device": [], "host": []}
        got = {}
        for _ in range(3):
            for mode in ("device", "host"):
                if mode == "host":
                    os.environ["GS_HOST_FAST"] = "0"
                t0 = time.perf_counter()
                m, tot = host.accmap_files([path], known, CATEGORIES, STATUSES, "ALL", reserve_entries=n // 8)
                t[mode].append(time.perf_counter() - t0)
                os.environ.pop("GS_HOST_FAST", None)
                assert (tot["device_chunks"] > 0) == (mode == "device")
                got[mode] = (tot["passing"], tot["put"], m.fetch()[1][:1000].tolist())
                m.close()
        assert got["device"] == got["host"]
        print(f"gs_host_accmap_files, {name} file: device path {min(t['device']):.3f} s (slowest {max(t['device']):.3f}), GS_HOST_FAST=0 "
              f"{min(t['host']):.3f} s (slowest {max(t['host']):.3f}); {tot['lines']} lines, {tot['passing']} pass, {tot['put']} put")
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
