"""Rates of the fastasgenbank goal.

    python tools/asmsum_rate.py [lines]

A generated assembly summary of `lines` lines (default 1 000 000; one chunk holds at most 1 GiB) in NCBI's layout of 38 columns, with
non-ASCII submitter names, drawn from a pool of 65 536 lines; four tax ids in five name a node of a tree of 20 000.
* between events (gs_asmsum_kernel_time), the chunk resident in device memory, five timed turns after one untimed, the fastest and
  the spread: the passes of a submit (tiles, slots, judge, write, gather) with the reference's default qualities and with every
  quality allowed, and the finish (the cap with genbank.maxPerTaxid 1); the fetch on the host clock;
* beside them, on the same bytes, the yardstick that exists in the parent: the passes of gs_accmap_submit (no line of a summary
  passes the catalog's prefix rule, so its write pass has nothing to store and is not launched: this is its count pass);
* the goal end to end from a plain and a .gz file (gs_host_asmsum_files), device path against GS_HOST_FAST=0 (the record-by-record
  parser), by turns, on the host clock."""
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

SUBMITTERS = ["Institut für Mikrobiologie", "Université de Montréal", "DOE Joint Genome Institute", "北京大学", "Broad Institute", "Wellcome Sanger Institute"]
LEVELS = ["Complete Genome", "Chromosome", "Scaffold", "Scaffold", "Contig", "Contig", "Contig"]


def text(n):
    rng = np.random.default_rng(17)
    known = np.unique(rng.integers(2, 3000000, 20000)).astype(np.int32)
    pool = []
    for i in range(65536):
        taxid = int(known[int(rng.integers(0, len(known)))]) if rng.random() < 0.8 else int(rng.integers(3000000, 4000000))
        species = int(known[int(rng.integers(0, len(known)))]) if rng.random() < 0.8 else taxid
        acc, asm = "GCA_%09d.%d" % (i, 1 + i % 3), "ASM%dv%d" % (int(rng.integers(1000, 999999)), 1 + i % 2)
        f = [acc, "PRJNA%d" % int(rng.integers(1, 999999)), "SAMN%08d" % int(rng.integers(1, 99999999)), "", ["reference genome", "representative genome", "na", "na"][i & 3],
             str(taxid), str(species), "Escherichia coli str. K-12 substr. MG1655" + "x" * int(rng.integers(0, 60)), "strain=K-12", "",
             ["latest", "latest", "latest", "replaced", "suppressed"][i % 5], LEVELS[int(rng.integers(0, len(LEVELS)))], "Major", "Full", "2020/01/01", asm,
             SUBMITTERS[i % len(SUBMITTERS)], "GCF_%09d.%d" % (i, 1), "identical",
             "https://ftp.ncbi.nlm.nih.gov/genomes/all/GCA/%03d/%03d/%03d/%s_%s" % (i // 1000000 % 1000, i // 1000 % 1000, i % 1000, acc, asm), "", "na",
             "assembly from type material" if i % 9 == 0 else "na", "haploid", "bacteria", str(int(rng.integers(100000, 9999999))),
             str(int(rng.integers(100000, 9999999))), "50.5", "1", "1", str(int(rng.integers(1, 300))), "NCBI Prokaryotic Genome Annotation Pipeline (PGAP)",
             "2020/01/01", "4500", "4300", "80", "na", "na"]
        pool.append(("\t".join(f) + "\n").encode("utf-8"))
    return b"".join(pool[i] for i in rng.integers(0, len(pool), n)), known


def turns(run, label, mb=None):
    """one untimed and five timed turns of run() -> milliseconds per turn; prints the fastest and the spread"""
    run()
    ms = sorted(run() for _ in range(5))
    rate = f" = {mb / ms[0]:.1f} GB/s of text" if mb else ""
    print(f"{label}: {ms[0]:.3f} ms fastest of 5 (slowest {ms[-1]:.3f}){rate}", flush=True)
    return ms[0]


def main():
    import torch

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    data, known = text(n)
    mb = len(data) / 1e6
    print(f"{n} lines, {mb:.1f} MB", flush=True)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    state = {}

    def timed(m, what):
        before = m.kernel_time(True)[1]
        what()
        return m.kernel_time(True)[1] - before

    def submit(qualities):
        if state.get("h"):
            state["h"].close()
        h = state["h"] = ga.DeviceAssemblySummary(known, qualities=qualities, reserve_entries=n)
        return timed(h, lambda: state.update(rep=h.submit(dev, last=True)))

    def finish():
        submit(None)
        return timed(state["h"], lambda: state.update(info=state["h"].finish(1)))

    t_default = turns(lambda: submit(("COMPLETE_LATEST", "CHROMOSOME_LATEST")), "submit, default qualities (tiles, slots, judge, write, gather)", mb)
    rep = state["rep"]
    assert rep["refused"] == 0
    print(f"  {rep['counted']} counted, {rep['kept']} kept, {rep['pool_bytes']} pool bytes, longest line {rep['longest_line']}")
    t_all = turns(lambda: submit(None), "submit, every quality allowed", mb)
    rep = state["rep"]
    print(f"  {rep['counted']} counted, {rep['kept']} kept, {rep['pool_bytes']} pool bytes")
    turns(finish, "finish (the cap with max 1: counts, two scans, one sort, place, pick)")
    print("  kept %d, picked %d, nodes with entries %d, counted %d" % state["info"])

    def fetch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        state["picks"] = state["h"].fetch()
        return (time.perf_counter() - t0) * 1e3
    turns(fetch, "fetch of the picks into Python objects (host clock)")
    state["h"].close()

    # the yardstick on the same bytes
    def accmap():
        m = ga.DeviceAccessionMap(known, ["bacteria"], ["latest"], "ALL")
        ms = timed(m, lambda: state.update(arep=m.submit(dev, last=True)))
        m.close()
        return ms
    t_acc = turns(accmap, "yardstick, gs_accmap submit on the same bytes (count pass; nothing passes, no write pass)", mb)
    assert state["arep"]["refused"] == 0, state["arep"]
    print(f"  submit over yardstick: default {t_default / t_acc:.2f}x, every quality {t_all / t_acc:.2f}x")

    # end to end: gs_host_asmsum_files from a plain and a .gz file, the device path by turns with GS_HOST_FAST=0, on the host clock
    tmp = tempfile.mkdtemp()
    plain, gz = os.path.join(tmp, "assembly_summary.txt"), os.path.join(tmp, "assembly_summary.txt.gz")
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
                picks, total, tot = host.assembly_summary_files([path], known)
                t[mode].append(time.perf_counter() - t0)
                os.environ.pop("GS_HOST_FAST", None)
                assert (tot["device_chunks"] > 0) == (mode == "device")
                got[mode] = (total, tot["kept"], tot["picked"], sorted(picks)[:1000], [picks[k][0]["line"] for k in sorted(picks)[:1000]])
        assert got["device"] == got["host"]
        print(f"gs_host_asmsum_files, {name} file: device path {min(t['device']):.3f} s (slowest {max(t['device']):.3f}), GS_HOST_FAST=0 "
              f"{min(t['host']):.3f} s (slowest {max(t['host']):.3f}); {tot['lines']} lines, {tot['counted']} counted, {tot['kept']} kept, "
              f"{tot['picked']} picked", flush=True)
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
