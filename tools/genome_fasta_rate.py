"""Genome FASTA text -> build regions (developer tool): the kernels of gs_genomes alone, and files through
gs_host_genome_files into gs_dbbuild_add, on the synthetic collection tools/build_db_rate.py uses.

    python tools/genome_fasta_rate.py [genera] [rounds] [parts]      (20 species per genus, 100 kbp each; default 25 genera, 5 rounds,
                                                                      parts kernels,files,into)

1. Kernels alone, between events on the handle's stream (DeviceGenomes.kernel_time), the text resident on the device: scan and
   select + gather as GB/s of TEXT for 60-base LF lines, 80-base CRLF lines and unwrapped records, keep = all and one in ten;
   beside them gs_build_kmers_kernel on the gathered bases (the k-mer time of a DeviceDbUpdater over a one-k-mer store), the
   kernel this stage feeds, and the FASTA text stage of the read goals on the same text (gs_reads_select_fasta, every record).
2. File to builder: a plain, a gzip and a BGZF file of the 60-base text through host.genome_files into DeviceDbBuilder.add (fill
   walk), against a Python line loop that feeds the same builder from host memory (what examples/build_db.py did), and against
   the line-by-line parser of the host layer forced for every chunk (GS_HOST_FAST=0).
3. Callbacks or none: the plain file into DeviceDbBuilder.add through host.genome_files_into (an accession map on the device, a
   table of value indices, no callback) and through host.genome_files with its two ctypes callbacks, by turns.  They share one
   loop: the expectation is equality within the spread of the runs.
Every figure: the fastest of `rounds` runs taken by turns, with the spread (slowest / fastest - 1).  One JSON line per part."""
import ctypes as C
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host, synth  # noqa: E402


def fasta_text(genomes, width, eol):
    out = []
    for i in range(genomes.shape[0]):
        body = genomes[i].tobytes()
        out.append(b">g%d|synthetic genome %d" % (i, i) + eol)
        if width:
            out.append(eol.join(body[j:j + width] for j in range(0, len(body), width)) + eol)
        else:
            out.append(body + eol)
    return b"".join(out)


def best(xs):
    return {"best": round(min(xs), 4), "spread": round(max(xs) / min(xs) - 1, 3)}


def read_fasta(path):
    """the Python loop examples/build_db.py read its files with"""
    out, name, parts = [], None, []
    with open(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if name is not None:
                    out.append((name, b"".join(parts)))
                name, parts = line[1:].strip(), []
            elif name is not None:
                parts.append(line.rstrip(b"\r\n"))
    if name is not None:
        out.append((name, b"".join(parts)))
    return out


def main():
    genera = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    parts = sys.argv[3].split(",") if len(sys.argv) > 3 else ["kernels", "files", "into"]
    db = synth.SynthDB(genera=genera, species_per_genus=20)
    n_gen, bases = db.genomes.shape[0], int(db.genomes.size)
    shapes = {"lf60": fasta_text(db.genomes, 60, b"\n"), "crlf80": fasta_text(db.genomes, 80, b"\r\n"), "unwrapped": fasta_text(db.genomes, 0, b"\n")}
    keeps = {"all": None, "one_in_ten": np.arange(n_gen) % 10 == 0}

    if "kernels" in parts:
        kernels_alone(db, shapes, keeps, rounds)
    if "files" in parts:
        file_to_builder(db, shapes["lf60"], rounds)
    if "into" in parts:
        callbacks_or_none(db, shapes["lf60"], rounds)


def kernels_alone(db, shapes, keeps, rounds):
    n_gen, bases = db.genomes.shape[0], int(db.genomes.size)
    g = ga.DeviceGenomes()
    upd = ga.DeviceDbUpdater.from_arrays(31, db.kmers[:1], db.value_idx[:1], db.n_values, db.parent_vi)
    dev = {name: torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for name, t in shapes.items()}
    torch.cuda.synchronize()
    ms = {(s, k): {"scan": [], "gather": [], "kmers": []} for s in shapes for k in keeps}
    for r in range(rounds + 1):  # (round 0 warms every shape up: code objects, buffers at their final size)
        for s in shapes:
            for k, keep in keeps.items():
                a0, b0 = g.kernel_time()
                g.scan(dev[s], True)
                g.gather(keep)
                a1, b1 = g.kernel_time()
                seq, off = g.regions()
                nodes = db.species_vi if keep is None else db.species_vi[keep]
                k0 = upd.stats().ms_kmers
                upd.add(seq, off, nodes)
                k1 = upd.stats().ms_kmers
                if r:
                    ms[(s, k)]["scan"].append(a1 - a0)
                    ms[(s, k)]["gather"].append(b1 - b0)
                    ms[(s, k)]["kmers"].append(k1 - k0)
    # the nearest existing kernel family on the same text: the FASTA text stage of the read goals (gs_reads_select_fasta: newline
    # scan, record search, gather of the sequence lines, selection by descriptor), a chunk from its submission to its flags
    # between events (gs_reads_phase_times[0]).  It keeps every record and takes the text as one chunk of whole records.
    reads = ga.DeviceReads(k=31)
    L = ga.lib()
    key = np.frombuffer(b"g", dtype=np.uint8)
    acc = torch.zeros(n_gen, dtype=torch.uint8, device="cuda:0")
    reads_ms = {s: [] for s in shapes}
    reads_note = {}
    reads.kernel_time(True)
    for r in range(rounds + 1):
        for s, t in shapes.items():
            n_lines = t.count(b"\n")
            acc.zero_()
            torch.cuda.synchronize()
            before = reads.phase_times()["select"]
            rc = L.gs_reads_select_fasta(reads.h, 31, C.c_void_p(dev[s].data_ptr()), len(t), n_lines, n_gen, ga.MEM_DEVICE,
                                         key.ctypes.data_as(C.c_void_p), 1, C.c_void_p(acc.data_ptr()), None, None)
            if rc != 0 or L.gs_reads_sync(reads.h) != 0 or int(acc.sum().item()) != n_gen:  # (">g...": every record is accepted if the chunk was taken)
                reads_note[s] = "not taken: " + (L.gs_last_error() or b"refused by the text stage").decode(errors="replace")
                reads.text_reset(True)
                continue
            after = reads.phase_times()["select"]
            if r:
                reads_ms[s].append(after[1] - before[1])
    reads.close()
    rows = []
    for (s, k), m in ms.items():
        text_gb = len(shapes[s]) / 1e9
        kept = bases if keeps[k] is None else int(keeps[k].sum()) * db.genomes.shape[1]
        rows.append({"shape": s, "keep": k, "text_mb": round(text_gb * 1e3, 1), "kept_mbases": round(kept / 1e6, 1),
                     "scan_ms": best(m["scan"]), "gather_ms": best(m["gather"]), "kmers_ms": best(m["kmers"]),
                     "reads_fasta_stage_ms": best(reads_ms[s]) if reads_ms[s] else reads_note.get(s),
                     "reads_fasta_stage_gb_s_text": round(text_gb / min(reads_ms[s]) * 1e3, 1) if reads_ms[s] else None,
                     "scan_gb_s_text": round(text_gb / min(m["scan"]) * 1e3, 1), "gather_gb_s_text": round(text_gb / min(m["gather"]) * 1e3, 1),
                     "scan_plus_gather_gb_s_text": round(text_gb / (min(m["scan"]) + min(m["gather"])) * 1e3, 1),
                     "kmers_gb_s_bases": round(kept / 1e9 / min(m["kmers"]) * 1e3, 1)})
    print(json.dumps({"part": "kernels", "genomes": n_gen, "bases": bases, "rounds": rounds, "rows": rows}), flush=True)
    g.close()
    upd.close()
    del dev



def file_to_builder(db, text, rounds):
    n_gen, bases = db.genomes.shape[0], int(db.genomes.size)
    with tempfile.TemporaryDirectory() as tmp:
        files = {"plain": os.path.join(tmp, "g.fasta"), "gzip": os.path.join(tmp, "g.gz.fasta.gz"), "bgzf": os.path.join(tmp, "g.bgzf.fasta.gz")}
        open(files["plain"], "wb").write(text)
        open(files["gzip"], "wb").write(gzip.compress(text, 1))
        open(files["bgzf"], "wb").write(bytes(ga.deflate_device(text)))
        vi_of = {b"g%d" % i: int(db.species_vi[i]) for i in range(n_gen)}
        resolve = lambda f, first, headers: [vi_of[h[1:].split(b"|")[0]] for h in headers]

        def through_files(path, fast):
            os.environ["GS_HOST_FAST"] = "1" if fast else "0"
            b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
            t0 = time.time()
            t = host.genome_files([path], resolve, lambda s, o, v: b.add(s, o, v))
            dt = time.time() - t0
            b.close()
            os.environ.pop("GS_HOST_FAST")
            assert t.kept_bases == bases and (t.host_chunks == 0) == fast, (t.kept_bases, t.host_chunks)
            return dt

        def python_loop(path):
            b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
            t0 = time.time()
            recs = read_fasta(path)
            seq = np.frombuffer(b"".join(s for _, s in recs), dtype=np.uint8)
            off = np.cumsum([0] + [len(s) for _, s in recs]).astype(np.uint64)
            b.add(seq, off, np.array([vi_of[n.split(b"|")[0]] for n, _ in recs], np.int32))
            dt = time.time() - t0
            b.close()
            return dt

        ways = {"genome_files plain": lambda: through_files(files["plain"], True), "genome_files gzip": lambda: through_files(files["gzip"], True),
                "genome_files bgzf": lambda: through_files(files["bgzf"], True), "python loop plain": lambda: python_loop(files["plain"]),
                "host parser plain": lambda: through_files(files["plain"], False)}
        secs = {w: [] for w in ways}
        for r in range(min(rounds, 3) + 1):
            for w, fn in ways.items():
                dt = fn()
                if r:
                    secs[w].append(dt)
        out = {w: dict(best(v), mbases_per_s=round(bases / min(v) / 1e6, 1)) for w, v in secs.items()}
        print(json.dumps({"part": "file_to_builder", "text_mb": round(len(text) / 1e6, 1), "bases": bases, "seconds": out}), flush=True)


def callbacks_or_none(db, text, rounds):
    n_gen, bases = db.genomes.shape[0], int(db.genomes.size)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "g.fasta")
        open(path, "wb").write(text)
        # node i = genome i; the accession of ">g7|synthetic genome 7" is what stands in front of the first blank
        amap = ga.DeviceAccessionMap(np.arange(1, n_gen + 1), ["x"], ["x"])
        amap.append([b"g%d|synthetic" % i for i in range(n_gen)], np.arange(n_gen))
        amap.finish()
        vi_of_node = np.ascontiguousarray(db.species_vi, dtype=np.int32)
        vi_of = {b"g%d" % i: int(db.species_vi[i]) for i in range(n_gen)}
        resolve = lambda f, first, headers: [vi_of[h[1:].split(b"|")[0]] for h in headers]

        def run(into):
            b = ga.DeviceDbBuilder(31, db.n_values, db.parent_vi)
            t0 = time.time()
            if into:
                t = host.genome_files_into([path], b, vi_of_node, accession_map=amap)
            else:
                t = host.genome_files([path], resolve, lambda s, o, v: b.add(s, o, v))
            dt = time.time() - t0
            b.close()
            assert t.kept_bases == bases and t.kept_records == n_gen and t.host_chunks == 0, (t.kept_bases, t.kept_records, t.host_chunks)
            return dt

        secs = {"genome_files_into": [], "genome_files with callbacks": []}
        for r in range(rounds + 1):  # (round 0 warms up)
            for w in secs:
                dt = run(w == "genome_files_into")
                if r:
                    secs[w].append(dt)
        amap.close()
        out = {w: {"fastest": round(min(v), 4), "slowest": round(max(v), 4), "mbases_per_s": round(bases / min(v) / 1e6, 1)} for w, v in secs.items()}
        print(json.dumps({"part": "callbacks_or_none", "text_mb": round(len(text) / 1e6, 1), "bases": bases, "runs": rounds, "seconds": out}), flush=True)


if __name__ == "__main__":
    main()
