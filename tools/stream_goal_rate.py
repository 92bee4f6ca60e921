"""Rates of the two read-stream goals, extract and fasta2fastq.

    python tools/stream_goal_rate.py [reads] [--records]

* the FASTA -> FASTQ text kernels alone (sizes, offsets, copy between events: gs_reads_kernel_time), goal mode and ReadEntry
  mode, as GB/s of text written -- and, as a yardstick in the same session, the wall time of the existing four-line gather
  (gs_filter_compact_text, every record accepted) against the wall time of the same call on the new handle for FASTA text of the
  same size;
* both goals end to end for plain, gzip and BGZF input into a .gz output, device path against the host layer's reference-exact
  path (GS_HOST_FAST=0) of the same build, alternating -- and, from one further run of the device path in a process of its own
  with GS_HOST_TRACE set, where the time goes: the phases of the host layer's file loop and, between events on the handle's
  stream, the select stage, the four-line gather and the FASTA -> FASTQ text kernels (gs_reads_phase_times);
* extract of a plain FASTA file and of a plain general FASTQ file (sequence and quality over two lines each) into a .gz output,
  the records written on the device against GS_DEVICE_RECORDS=0 (the host's formatter and zlib), alternating, three runs each --
  and the text kernels of gs_reads_compact_records between events for both chunk kinds beside the four-line gather of text of the
  same size.  --records: these rows only."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host  # noqa: E402

READ = 150


def texts(n):
    rng = np.random.default_rng(5)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n * READ)].reshape(n, READ)
    fq, fa, ml = [], [], []
    for i in range(n):
        s = seq[i].tobytes()
        d = b"s%d:%d run" % (i % 8, i)
        fq.append(b"@" + d + b"\n" + s + b"\n+\n" + b"I" * READ + b"\n")
        fa.append(b">" + d + b"\n" + s[:75] + b"\n" + s[75:] + b"\n")
        ml.append(b"@" + d + b"\n" + s[:75] + b"\n" + s[75:] + b"\n+\n" + b"I" * 75 + b"\n" + b"J" * 75 + b"\n")
    return b"".join(fq), b"".join(fa), b"".join(ml)


def record_rows(n, fq, fa, ml, tmp):
    """extract of FASTA and general FASTQ into .gz, device records against GS_DEVICE_RECORDS=0; the text kernels between events"""
    gbp = n * READ / 1e9
    for kind, data in (("fasta", fa), ("multi-line fastq", ml)):
        src = os.path.join(tmp, "records." + ("fasta" if kind == "fasta" else "fastq"))
        open(src, "wb").write(data)
        t = {"device": [], "host": []}
        for _ in range(3):
            for mode in ("device", "host"):
                if mode == "host":
                    os.environ["GS_DEVICE_RECORDS"] = "0"
                before = host.stat(3)
                t0 = time.perf_counter()
                run_goal("extract", src, os.path.join(tmp, f"records_{mode}.fastq.gz"))
                t[mode].append(time.perf_counter() - t0)
                assert (host.stat(3) > before) == (mode == "device")
                os.environ.pop("GS_DEVICE_RECORDS", None)
        same = gzip.open(os.path.join(tmp, "records_device.fastq.gz")).read() == gzip.open(os.path.join(tmp, "records_host.fastq.gz")).read()
        fmt = lambda ts: " / ".join(f"{x * 1e3:.0f}" for x in ts)
        print(f"extract plain {kind} -> .gz: records on the device {fmt(t['device'])} ms ({gbp / min(t['device']):.2f} Gbp/s), "
              f"GS_DEVICE_RECORDS=0 {fmt(t['host'])} ms ({gbp / min(t['host']):.2f} Gbp/s), same text: {same}")
        print("  " + phases("extract", src, os.path.join(tmp, "records_traced.fastq.gz")))
    # the text kernels: every record selected, qualities on
    reads = ga.DeviceReads(k=31)
    reads.kernel_time(True)
    for kind, select, data in (("FASTA", reads.select_fasta, fa), ("multi-line FASTQ, qualities gathered", reads.select_fastq_ml, ml)):
        select(data, b"s")
        nbytes = len(reads.compact_records(True)[0])
        n0, ms0 = reads.kernel_time(True)
        for i in range(5):
            select(data, b"s")  # (a new chunk: the quality gather runs once per chunk)
            reads.compact_records(True, i & 1)
        n1, ms1 = reads.kernel_time(True)
        per = (ms1 - ms0) / (n1 - n0)
        print(f"gs_reads_compact_records, {kind}: text kernels {per:.3f} ms = {nbytes / per / 1e6:.1f} GB/s of {nbytes / 1e6:.1f} MB written")
    reads.select_text(fq, b"s")
    L = ga.lib()
    p, nb, nr = C.c_void_p(), C.c_int64(0), C.c_int64(0)

    def gather():
        assert L.gs_reads_compact_text(reads.h, 1, 0, C.byref(p), C.byref(nb), C.byref(nr)) == 0

    gather()
    t = min(best(gather, 3)[0] for _ in range(3))
    print(f"yardstick, four-line gather (gs_reads_compact_text): {nb.value / 1e6:.1f} MB, call wall min {t * 1e3:.3f} ms = {nb.value / t / 1e9:.1f} GB/s")


def bgzf(data, block=65280):
    """block gzip as bgzip writes it: members of at most 64 KiB of text whose extra field gives their size, and the empty last one"""
    out = []
    for i in list(range(0, len(data), block)) + [len(data)]:
        c = data[i:i + block]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = z.compress(c) + z.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<HccHH", 6, b"B", b"C", 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(c), len(c)))
    return b"".join(out)


def run_goal(goal_name, src, dst):
    if goal_name == "extract":
        return host.extract_files(b"s3:", [src], dst)
    return host.fasta2fastq([src], dst)


def phases(goal_name, src, dst):
    """the `<goal> phases:` line of the second of two runs of the device path in a fresh process (the trace switch is read once
    per process)"""
    env = dict(os.environ, GS_HOST_TRACE="1")
    env.pop("GS_HOST_FAST", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", goal_name, src, dst], env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith(goal_name + " phases:")]
    return lines[-1] if r.returncode == 0 and lines else f"{goal_name} phases: not reported (exit {r.returncode})"


def best(f, rounds=7):
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--one":
        for _ in range(2):  # (the second run is the one reported: the first one of a process pays for its allocations)
            run_goal(*sys.argv[2:])
        return
    args = [a for a in sys.argv[1:] if a != "--records"]
    n = int(args[0]) if args else 1_000_000
    fq, fa, ml = texts(n)
    print(f"{n} reads of {READ} bases: FASTQ {len(fq) / 1e6:.1f} MB, FASTA {len(fa) / 1e6:.1f} MB, multi-line FASTQ {len(ml) / 1e6:.1f} MB")
    if "--records" in sys.argv[1:]:
        record_rows(n, fq, fa, ml, tempfile.mkdtemp())
        return
    L = ga.lib()
    reads = ga.DeviceReads(k=31)
    reads.kernel_time(True)
    out_bytes = {}

    def kernel_rate(name, call):
        call()
        n0, ms0 = reads.kernel_time(True)
        wall = best(call)
        n1, ms1 = reads.kernel_time(True)
        per = (ms1 - ms0) / (n1 - n0)
        print(f"{name}: text kernels {per:.3f} ms = {out_bytes[name] / per / 1e6:.1f} GB/s of {out_bytes[name] / 1e6:.1f} MB written; "
              f"call wall min {wall[0] * 1e3:.2f} ms, median {wall[1] * 1e3:.2f} ms")

    def goal():
        out_bytes["fasta2fastq (goal mode)"] = len(reads.fasta2fastq(fa)[0])

    def entry():
        out_bytes["extract FASTA (ReadEntry mode)"] = len(reads.compact_text()[0])

    kernel_rate("fasta2fastq (goal mode)", goal)
    reads.select_fasta(fa, b"s")
    kernel_rate("extract FASTA (ReadEntry mode)", entry)

    # the yardstick: gather calls alone (no fetch), all records selected, interleaved
    bloom = ga.DeviceBloomFilter(ga.BLOOM_XOR, 64, [1], np.zeros(1, np.uint64))
    f = ga.FastqBloomFilter(31, bloom)
    f.positive_ratio, f.min_pos_count = 0.0, 0
    acc = np.zeros(n, dtype=np.uint8)
    f.submit_text(fq, acc)
    f.sync()
    reads.select_text(fq, b"s")
    reads2 = ga.DeviceReads(k=31)
    reads2.select_fasta(fa, b"s")
    p, nb, nr = C.c_void_p(), C.c_int64(0), C.c_int64(0)

    def gather_filter():
        assert L.gs_filter_compact_text(bloom.h, 0 if acc.sum() == 0 else 1, 0, 0, C.byref(p), C.byref(nb), C.byref(nr)) == 0
        return nb.value

    def gather_reads():
        assert L.gs_reads_compact_text(reads.h, 0, 0, C.byref(p), C.byref(nb), C.byref(nr)) == 0
        return nb.value

    def gather_fasta():
        assert L.gs_reads_compact_text(reads2.h, 0, 0, C.byref(p), C.byref(nb), C.byref(nr)) == 0
        return nb.value

    for name, g in (("four-line gather (gs_filter_compact_text)", gather_filter), ("four-line gather (gs_reads_compact_text)", gather_reads),
                    ("FASTA -> FASTQ, ReadEntry mode (gs_reads_compact_text)", gather_fasta)):
        nbytes = g()
        rounds = [best(g, 3) for _ in range(3)]
        t = min(r[0] for r in rounds)
        print(f"{name}: {nbytes / 1e6:.1f} MB, call wall min {t * 1e3:.3f} ms = {nbytes / t / 1e9:.1f} GB/s")

    # end to end
    tmp = tempfile.mkdtemp()
    for kind, pack in (("plain", lambda d: d), ("gzip", lambda d: gzip.compress(d, 1)), ("bgzf", bgzf)):
        suffix = "" if kind == "plain" else ".gz"
        pq, pa = os.path.join(tmp, f"{kind}.fastq{suffix}"), os.path.join(tmp, f"{kind}.fasta{suffix}")
        open(pq, "wb").write(pack(fq))
        open(pa, "wb").write(pack(fa))
        for goal_name, src in (("extract", pq), ("fasta2fastq", pa)):
            t = {"device": [], "cpu": []}
            for _ in range(3):
                for mode in ("device", "cpu"):
                    if mode == "cpu":
                        os.environ["GS_HOST_FAST"] = "0"
                    t0 = time.perf_counter()
                    run_goal(goal_name, src, os.path.join(tmp, f"{goal_name}_{mode}.fastq.gz"))
                    t[mode].append(time.perf_counter() - t0)
                    os.environ.pop("GS_HOST_FAST", None)
            same = gzip.open(os.path.join(tmp, f"{goal_name}_device.fastq.gz")).read() == gzip.open(os.path.join(tmp, f"{goal_name}_cpu.fastq.gz")).read()
            gbp = n * READ / 1e9
            print(f"{goal_name} {kind} -> .gz: device {gbp / min(t['device']):.2f} Gbp/s ({min(t['device']) * 1e3:.0f} ms), "
                  f"cpu path {gbp / min(t['cpu']):.2f} Gbp/s ({min(t['cpu']) * 1e3:.0f} ms), same text: {same}")
            print("  " + phases(goal_name, src, os.path.join(tmp, f"{goal_name}_traced.fastq.gz")))
    record_rows(n, fq, fa, ml, tmp)


if __name__ == "__main__":
    main()
