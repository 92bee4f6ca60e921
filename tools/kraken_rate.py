"""end-to-end rate of gs_host_match_files with per-read outputs (Kraken-style lines, filtered FASTQ), and the device time of the
text kernels that write the lines (developer tool)

    kraken_rate.py [reads] [gz] [--repeats N] [--shape four-line|fasta|multi-line]

--shape: the input file's records -- four lines each (the default), FASTA with the read over two lines, or general FASTQ with the read
and its qualities over two lines each (per-read outputs of the last two: the record kernels, GS_DEVICE_RECORDS=0 the host formatter).

Every row is run N times (the rows by turns); the summary gives the fastest run and the spread (slowest - fastest) of each row."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import host, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("reads", nargs="?", type=int, default=2_000_000)
ap.add_argument("gz", nargs="?", default="", help="'gz': compressed outputs (multi-member gzip)")
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--shape", choices=("four-line", "fasta", "multi-line"), default="four-line")
args = ap.parse_args()
n = args.reads
gz = ".gz" if args.gz == "gz" else ""
db = synth.SynthDB()
store = ga.DeviceKMerStore(31, db.kmers, db.value_idx, db.n_values, db.parent_vi)
seq, off = synth.reads_host(db.genomes, n)
d = tempfile.mkdtemp(prefix="gskr")
path = os.path.join(d, "reads.fasta" if args.shape == "fasta" else "reads.fastq")
L = 150
H = L // 2
blk = seq.tobytes()
if args.shape == "fasta":
    record = lambda i: b">r%d\n" % i + blk[i * L:i * L + H] + b"\n" + blk[i * L + H:(i + 1) * L] + b"\n"
elif args.shape == "multi-line":
    record = lambda i: b"@r%d\n" % i + blk[i * L:i * L + H] + b"\n" + blk[i * L + H:(i + 1) * L] + b"\n+\n" + b"I" * H + b"\n" + b"I" * (L - H) + b"\n"
else:
    record = lambda i: b"@r%d\n" % i + blk[i * L:(i + 1) * L] + b"\n+\n" + b"I" * L + b"\n"
with open(path, "wb") as f:
    f.write(b"".join(record(i) for i in range(n)))
rows = (("table only", {}), ("kraken out", dict(kraken_out_path=os.path.join(d, "k.out" + gz), taxids=db.taxids)),
        ("filtered fastq", dict(filtered_path=os.path.join(d, "f.fastq" + gz))),
        ("both", dict(kraken_out_path=os.path.join(d, "k.out" + gz), taxids=db.taxids, filtered_path=os.path.join(d, "f.fastq" + gz))))
times = {label: [] for label, _ in rows}
for rep in range(max(args.repeats, 1)):
    for label, kw in rows:
        t0 = time.perf_counter()
        _, _, tot = host.match_files(store, [path], **kw)
        dt = time.perf_counter() - t0
        times[label].append(dt)
        print(f"{label:15s}: {dt:.2f} s -> {n * 150 / dt / 1e9:.3f} Gbp/s (parse {tot.seconds_parse:.2f} s, gpu {tot.seconds_gpu:.2f} s)", flush=True)
for label, _ in rows:
    t = times[label]
    print(f"summary {label:15s}: min {min(t):.3f} s = {n * 150 / min(t) / 1e9:.3f} Gbp/s, spread {max(t) - min(t):.3f} s over {len(t)} runs", flush=True)

# the text kernels of the lines between events (an event pair around the size pass and one around the write pass of every call): one
# chunk of up to 1 Mi reads, with the match kernel on the same chunk beside it
m = ga.FastqKMerMatcher(store, ga.MatchConfig(profile=True))
m.set_taxids(db.taxids)
nc = min(n, 1 << 20)
chunk = np.frombuffer(b"".join(record(i) for i in range(nc)), dtype=np.uint8)
cv, fl = np.zeros(2 * nc + 2, dtype=np.int32), np.zeros(2 * nc + 2, dtype=np.uint8)
calls = 5
k0 = m0 = 0.0
for call in range(calls + 1):  # (the first call sizes the buffers and is left out)
    if args.shape == "fasta":
        m.submit_fasta(chunk, n_lines=3 * nc, n_records=nc, class_vi=cv, flags=fl)
    elif args.shape == "multi-line":
        m.submit_fastq_ml(chunk, n_lines=6 * nc, class_vi=cv, flags=fl)
    else:
        m.submit_text(chunk, n_lines=4 * nc, class_vi=cv, flags=fl)
    text = m.kraken_text(True) if args.shape == "four-line" else m.kraken_records(True)
    if call == 0:
        k0, m0 = m.kraken_time()[1], m.kernel_time()[1]
k_ms, m_ms = (m.kraken_time()[1] - k0) / calls, (m.kernel_time()[1] - m0) / calls
print(f"lines on the device: {k_ms * 1e7 / nc:.2f} ms of text kernels per 10 M reads ({len(text) * 1e7 / nc / 1e6:.0f} MB of text, "
      f"{len(text) / (k_ms * 1e-3) / 1e9:.1f} GB/s written); match kernel on the same chunks: {m_ms * 1e7 / nc:.2f} ms per 10 M reads", flush=True)
m.close()
shutil.rmtree(d)
