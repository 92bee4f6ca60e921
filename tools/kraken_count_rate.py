"""Rates of the krakencount goal.

    python tools/kraken_count_rate.py [reads]

A synthetic Kraken-style file of `reads` lines (default 2 000 000: about half of all tokens on tax id 0, a handful of tax ids
the rest, some 'A' tokens).
* the kernels of gs_krakencount alone, the text in device memory, between events (gs_krakencount_kernel_time), as bytes of text
  per second -- and beside it, as the yardstick already in the tree, the four-line text stage of gs_reads on the same bytes from
  device memory between events (its newline scan and record check; the chunk is no FASTQ and is refused there);
* the global atomics the accumulation issued per token, from the handle's own counters;
* the goal end to end from a plain and a .gz file, device path against GS_HOST_FAST=0 (the line-by-line parser), by turns."""
import ctypes as C
import gzip
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host  # noqa: E402


def text(n):
    rng = np.random.default_rng(7)
    taxa = [562, 1280, 9606, 10239, 2697049, 1000, 100001]
    pool = []
    for i in range(4096):
        toks = []
        for _ in range(int(rng.integers(1, 6))):
            u = rng.random()
            key = b"0" if u < 0.5 else b"A" if u < 0.55 else b"%d" % taxa[int(rng.integers(0, 3 if u < 0.9 else len(taxa)))]
            toks.append(key + b":%d" % int(rng.integers(1, 121)))
        cls = taxa[int(rng.integers(0, 3))] if i % 3 else 0
        pool.append(b"%s\tA01245:102:HXXXX:1:%d:%d\t%d\t150\t%s\n" % (b"C" if cls else b"U", 1101 + i % 50, i, cls, b" ".join(toks)))
    return b"".join(pool[i] for i in rng.integers(0, len(pool), n))


def main():
    import torch

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
    data = text(n)
    mb = len(data) / 1e6
    print(f"{n} lines, {mb:.1f} MB")
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    kc = ga.KrakenCounter(0)
    kc.submit(dev)  # (buffers, warm-up)
    kc.reset()
    kc.kernel_time(True)
    for _ in range(5):
        rep = kc.chunk(kc.submit(dev))
        assert rep["refused"] == 0
    launches, ms = kc.kernel_time(False)
    tokens = kc.status()[3][1] + kc.status()[3][2]
    atomics, direct = kc.counters()
    per = ms / launches
    print(f"gs_krakencount kernels (count, scans, check, accumulate, commit): {per:.3f} ms per chunk = {mb / per:.1f} GB/s of text")
    print(f"global atomics of the accumulation: {atomics} for {tokens} tokens = {atomics / tokens:.5f} per token; {direct} tokens went straight to the global table")
    kc.close()
    # the yardstick: the four-line text stage on the same bytes
    reads = ga.DeviceReads(k=31)
    L = ga.lib()
    acc = torch.zeros(max(n // 4, 1), dtype=torch.uint8, device="cuda:0")
    key = np.frombuffer(b"x", dtype=np.uint8)
    nl = n & ~3
    cut = len(data) if nl == n else int(np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)[nl - 1]) + 1

    def scan():
        L.gs_reads_select_text(reads.h, 31, C.c_void_p(dev.data_ptr()), cut, nl, ga.MEM_DEVICE, key.ctypes.data_as(C.c_void_p), 1, C.c_void_p(acc.data_ptr()), None, None)
        L.gs_reads_sync(reads.h)
        reads.text_reset(True)
    scan()
    reads.kernel_time(True)
    before = reads.phase_times()["select"]
    for _ in range(5):
        scan()
    after = reads.phase_times()["select"]
    per_y = (after[1] - before[1]) / max(after[0] - before[0], 1)
    print(f"yardstick, gs_reads four-line text stage on the same bytes: {per_y:.3f} ms per chunk = {cut / 1e6 / per_y:.1f} GB/s")
    reads.close()
    # end to end
    tmp = tempfile.mkdtemp()
    plain, gz = os.path.join(tmp, "k.out"), os.path.join(tmp, "k.out.gz")
    open(plain, "wb").write(data)
    open(gz, "wb").write(gzip.compress(data, 1))
    for name, path in (("plain", plain), (".gz", gz)):
        t = {"device": [], "host": []}
        rows = {}
        for _ in range(3):
            for mode in ("device", "host"):
                if mode == "host":
                    os.environ["GS_HOST_FAST"] = "0"
                t0 = time.perf_counter()
                rows[mode], tot = host.kraken_count_files([path])
                t[mode].append(time.perf_counter() - t0)
                os.environ.pop("GS_HOST_FAST", None)
                assert (tot["device_chunks"] > 0) == (mode == "device")
        fmt = lambda ts: " / ".join(f"{x * 1e3:.0f}" for x in ts)
        print(f"krakencount {name}: device path {fmt(t['device'])} ms ({mb / 1e3 / min(t['device']):.2f} GB/s), GS_HOST_FAST=0 {fmt(t['host'])} ms "
              f"({mb / 1e3 / min(t['host']):.2f} GB/s), same rows: {rows['device'] == rows['host']}")


if __name__ == "__main__":
    main()
