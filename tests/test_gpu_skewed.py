"""Parity of the whole match result on skewed workloads (genestrip_amd/synth.py: SkewedDB, skewed_reads) against the oracle,
with the checker of tests/matchcheck.py: integer table, class, flags, max hit counts and every double-table cell.

Stores (value indices from the oracle's DBGoal restatement; the dominant species is the last value index, so that its hot row is
not in the first pass of the reduction over values):
  A  k 31  ~70 values      LDS counters, deferred statistics records, overflow table in use
  B  k 31  ~700 values     global counters over the stat copies, two reduce passes of GS_REDUCE_VALUES (640)
  C  k 31  ~3000 values    taxonomy outside LDS (GS_NV_TREE_LDS 2048), five reduce passes
  D  k 31  ~11000 values   above GS_STAT_REC_MAX_VALUES (10240): no deferred records
  E  k 17  ~70 values      table-only layout (k below GS_MIN_K 19)
Each case: one binary submission, the same reads as four-line FASTQ text, and three uneven shards on separate runs joined by
gs_match_merge; default configuration and one that counts only part of the reads (with per-k-mer hit counters).
Then the file pipeline: the CSV's double columns and the max-contig descriptors for four-line FASTQ, multi-line FASTQ and FASTA,
plain, gzip and BGZF.  Needs an MI355X: run with -m gpu."""
import gzip
import json

import numpy as np
import pytest

import genestrip_amd as ga
import matchcheck
from conftest import bgzf
from genestrip_amd import binding, host, synth
from oracle import gs_oracle as orc

pytestmark = pytest.mark.gpu

FIRST = 1000  # first read number of every case
STORES = {  # name: (k, SkewedDB arguments)
    "A": (31, dict(genera=3, species_per_genus=4, genome_len=300_000, strains=2, dominant_len=1000, n_values=70, seed=11)),
    "B": (31, dict(genera=3, species_per_genus=3, genome_len=150_000, strains=2, dominant_len=1000, n_values=700, seed=12)),
    "C": (31, dict(genera=3, species_per_genus=3, genome_len=150_000, strains=2, dominant_len=1000, n_values=3000, seed=13)),
    "D": (31, dict(genera=3, species_per_genus=3, genome_len=150_000, strains=2, dominant_len=1000, n_values=11000, seed=14)),
    "E": (17, dict(genera=3, species_per_genus=4, genome_len=150_000, strains=2, dominant_len=1000, n_values=70, seed=15)),
}
CONFIGS = {
    "default": dict(),
    "partial": dict(threshold=3, max_read_tax_err=0.1, max_read_class_err=0.3, max_paths=1, max_kmer_res_counts=5),
}
WORST = {}  # store -> largest |g - S| / ((n + 3) 2^-53 S) seen


class Store:
    def __init__(self, name):
        self.name = name
        self.k, args = STORES[name]
        self.db = synth.SkewedDB(**args)
        seq, off, nvi = self.db.regions()
        b = orc.DbBuild(self.k, self.db.n_values, self.db.parent_vi)
        b.fill(seq, off, nvi)
        b.optimize()
        b.update(seq, off, nvi)
        self.kmers, self.vidx = b.fetch()
        b.close()
        self.odb = orc.DB(self.k, self.kmers, self.vidx, self.db.n_values, self.db.parent_vi)
        self.dev = ga.DeviceKMerStore(self.k, self.kmers, self.vidx, self.db.n_values, self.db.parent_vi)
        self.internal = np.unique(self.db.parent_vi[self.db.parent_vi >= 0])

    def close(self):
        self.dev.close()


_STORES = {}


def _store(name):
    if name not in _STORES:
        _STORES[name] = Store(name)
    return _STORES[name]


@pytest.fixture(scope="module", autouse=True)
def _close_stores():
    yield
    for s in _STORES.values():
        s.close()
    _STORES.clear()
    print("\nSKEWED worst dtable ratio per store: " + json.dumps(WORST))


def _oracle(st, seq, off, cfg):
    run = orc.MatchRun(st.odb, **cfg)
    cv, fl, terms = run.submit_terms(seq, off, FIRST, threads=16)
    t, d = run.finish()
    o = dict(table=t, dtable=d, class_vi=cv, flags=fl, terms=terms)
    if cfg.get("max_kmer_res_counts"):
        o["max_counts"] = run.max_counts()
    run.close()
    return o


def _result(m, cv=None, fl=None):
    t, d = m.finish()
    g = dict(table=t, dtable=d, class_vi=cv, flags=fl)
    if m.config.max_kmer_res_counts:
        g["max_counts"] = m.max_counts()
    return g


def _run_case(st, seq, off, cuts, cfg, what):
    """oracle vs binary, text and sharded + merged submissions; returns (oracle result, worst ratio)"""
    n = len(off) - 1
    o = _oracle(st, seq, off, cfg)
    ref = matchcheck.dtable_reference(o["terms"], st.db.n_values)
    mc = ga.MatchConfig(**cfg)
    worst = 0.0
    m = ga.FastqKMerMatcher(st.dev, mc)
    cv, fl = m.match_reads(seq, off, FIRST)
    worst = max(worst, matchcheck.check_match(o, _result(m, cv, fl), f"{what} binary", ref=ref))
    m.reset()
    text = np.frombuffer(synth.fastq_text(seq, off), dtype=np.uint8)
    cv2 = np.zeros(n, dtype=np.int32)
    fl2 = np.zeros(n, dtype=np.uint8)
    m.submit_text(text, first_read_no=FIRST, class_vi=cv2, flags=fl2)
    m.sync()
    assert m.text_status()[0] == -1, what
    worst = max(worst, matchcheck.check_match(o, _result(m, cv2, fl2), f"{what} text", ref=ref))
    m.close()
    del text
    # three uneven shards, global read numbers, separate runs merged; after every shard the run names the holders of the
    # longest contigs -- the holder gs_match_finish reports at the end must have been named when its shard went in
    bounds = [0, *cuts, n]
    replicas = [ga.DeviceKMerStore(st.k, st.kmers, st.vidx, st.db.n_values, st.db.parent_vi) for _ in range(len(bounds) - 1)]
    runs = [ga.FastqKMerMatcher(r, mc) for r in replicas]  # (one unique-counting run per store)
    named = set()
    for m, a, b in zip(runs, bounds[:-1], bounds[1:]):
        o0 = int(off[a])
        m.submit(seq[o0:int(off[b])], off[a:b + 1] - np.uint64(o0), first_read_no=FIRST + a, n_reads=b - a)
        now = m.max_contig_reads()
        named |= {(v, int(r)) for v, r in enumerate(now) if FIRST + a <= r < FIRST + b}
    binding.merge_runs(runs)
    for i, m in enumerate(runs):  # every run holds the global state
        g = _result(m)
        worst = max(worst, matchcheck.check_match(o, g, f"{what} shards, run {i}", ref=ref))
    final = o["table"][:, orc.C_MAX_CONTIG_READ_NO]
    missing = [(v, int(r)) for v, r in enumerate(final) if r >= 0 and (v, int(r)) not in named]
    assert not missing, f"{what}: final max-contig holders never named after their shard: {missing[:6]}"
    assert np.array_equal(runs[0].max_contig_reads(), final), what
    for m, r in zip(runs, replicas):
        m.close()
        r.close()
    return o, worst


def _clean_coverage(st, info, k):
    """a lower bound of the hits of the dominant genome's most-hit k-mer: the reads that carry its text unchanged"""
    dom = len(st.db.genomes) - 1
    sel = (info["src"] == dom) & info["clean"] & (info["length"] >= k)
    cov = np.zeros(len(st.db.genomes[dom]) + 1, dtype=np.int64)
    np.add.at(cov, info["pos"][sel], 1)
    np.add.at(cov, info["pos"][sel] + info["length"][sel] - k + 1, -1)
    return int(np.cumsum(cov).max()) if sel.any() else 0


def _internal_share(st, o):
    counted = o["flags"] & orc.F_COUNTED != 0
    return float(np.isin(o["class_vi"][counted], st.internal).mean()) if counted.any() else 0.0


CASES = [("A", "dominated", 1_000_000), ("A", "background", 1_000_000), ("A", "ragged", 1_000_000),
         ("B", "combined", 200_000), ("C", "combined", 200_000), ("D", "combined", 200_000), ("E", "combined", 200_000)]


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{a}-{b}" for a, b, _ in CASES])
def test_skewed_parity(case):
    name, mix, n = CASES[case]
    st = _store(name)
    cuts = (int(n * 0.17), int(n * 0.83))
    seq, off, info = synth.skewed_reads(st.db, n, mix, seed=100 + case, cuts=cuts)
    info_db = st.dev.info
    report = dict(store=name, mix=mix, reads=n, n_values=st.db.n_values, n_stored=int(info_db.n_stored),
                  n_in_records=int(info_db.n_in_records))
    if name == "A":
        assert info_db.n_in_records < info_db.n_stored  # the overflow table is in use
    worst = 0.0
    for cname, cfg in CONFIGS.items():
        o, w = _run_case(st, seq, off, cuts, cfg, f"{name}/{mix}/{cname}")
        worst = max(worst, w)
        counted = o["flags"] & orc.F_COUNTED != 0
        report[cname] = dict(counted=int(counted.sum()), internal_share=round(_internal_share(st, o), 4), worst_ratio=w)
        if cname == "default":
            if mix == "dominated":
                reads = o["table"][:, orc.C_READS]
                assert reads[st.db.dominant_vi] >= 0.85 * reads.sum(), (reads[st.db.dominant_vi], reads.sum())
                report["dominant_share"] = round(float(reads[st.db.dominant_vi] / reads.sum()), 4)
            else:
                assert _internal_share(st, o) >= 0.20, report
            if mix in ("ragged", "combined"):
                pos = np.diff(off.astype(np.int64)) - st.k + 1
                found = o["flags"] & orc.F_FOUND != 0
                wide, long_ = int((found & (pos > 128) & (pos <= 256)).sum()), int((found & (pos > 256)).sum())
                assert wide > 1000 and long_ > 1000, (wide, long_)
                report["wide_reads"], report["long_reads"] = wide, long_
        else:
            assert 1000 < counted.sum() < 0.95 * (o["flags"] & orc.F_FOUND != 0).sum(), "only part of the reads are counted"
    hits = _clean_coverage(st, info, st.k)
    report["max_hits_at_least"] = hits
    if mix == "dominated":
        assert hits > 32767  # the per-k-mer counters wrap as Java shorts
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print("\nSKEWED " + json.dumps(report))


# ------------------------------------------------------------------ file pipeline: dtable and max-contig descriptors
def _fastq4(seq, off, names):
    return synth.fastq_text(seq, off, names)


def _fastq_ml(seq, off, names, width=60):
    """multi-line FASTQ: sequence and quality wrapped at `width`; every third quality line starts with '@'"""
    out = []
    for i in range(len(off) - 1):
        s = seq[int(off[i]):int(off[i + 1])].tobytes()
        q = bytearray(b"I" * len(s))
        for j in range(0, len(q), width * 3):
            q[j] = ord("@")
        out.append(b"@" + names[i] + b"\n" + b"".join(s[j:j + width] + b"\n" for j in range(0, len(s), width)) + b"+\n" +
                   b"".join(bytes(q[j:j + width]) + b"\n" for j in range(0, len(q), width)))
    return b"".join(out)


def _fasta(seq, off, names, width=70):
    out = []
    for i in range(len(off) - 1):
        s = seq[int(off[i]):int(off[i + 1])].tobytes()
        out.append(b">" + names[i] + b"\n" + b"".join(s[j:j + width] + b"\n" for j in range(0, len(s), width)))
    return b"".join(out)


def _check_files(st, paths, parts, fasta_flags, what):
    """run the files through host.match_files and check table, dtable and descriptors against the oracle over the same reads"""
    seqs, offs, heads = [], [], []
    for data, is_fa in zip(parts, fasta_flags):
        p = orc.parse_fastq(data, fasta=is_fa, k=st.k)
        seqs.append(p["seq"])
        offs.append(p["seq_off"])
        d, do = p["desc"], p["desc_off"]
        heads += [d[int(do[i]):int(do[i + 1])].tobytes() for i in range(int(p["n_reads"]))]
    seq = np.concatenate(seqs)
    base = np.cumsum([0] + [int(o[-1]) for o in offs[:-1]])
    off = np.concatenate([offs[0]] + [o[1:] + np.uint64(b) for o, b in zip(offs[1:], base[1:])])
    run = orc.MatchRun(st.odb)
    cv, fl, terms = run.submit_terms(seq, off, 0, threads=16)
    t, d = run.finish()
    table, dtable, tot, desc = host.match_files(st.dev, paths, max_contig_desc=True)
    assert tot.reads == len(off) - 1, what
    w = matchcheck.check_match(dict(table=t, dtable=d, terms=terms), dict(table=table, dtable=dtable), what)
    holder = t[:, orc.C_MAX_CONTIG_READ_NO]
    assert (holder >= 0).sum() > 10, what
    for v in range(st.db.n_values):
        r = int(holder[v])
        want = heads[r][1:].split(b" ", 1)[0].rstrip(b"\n") if r >= 0 else b""
        assert desc[v] == want, f"{what}: value {v} holder {r}: descriptor {desc[v]!r}, want {want!r}"
    return w


@pytest.fixture(scope="module")
def mix_files(tmp_path_factory):
    st = _store("A")
    n = 60_000
    seq, off, _ = synth.skewed_reads(st.db, n, "ragged", seed=77)
    names = [b"read%d/1 sample:%d length=%d" % (i, i % 7, int(off[i + 1] - off[i])) for i in range(n)]
    d = tmp_path_factory.mktemp("skewed_files")
    forms = {"fq": _fastq4(seq, off, names), "mlfq": _fastq_ml(seq, off, names), "fa": _fasta(seq, off, names)}
    half = n // 2
    forms["fq_head"] = _fastq4(seq[:int(off[half])], off[:half + 1], names[:half])
    forms["fa_tail"] = _fasta(seq[int(off[half]):], off[half:] - off[half], names[half:])
    paths = {}
    for key, data in forms.items():
        ext = ".fasta" if key.startswith("fa") else ".fastq"
        for comp, blob in (("", data), (".gz", gzip.compress(data, 1)), (".bgzf.gz", bgzf(data))):
            p = d / (f"{key}_bgzf{ext}.gz" if comp == ".bgzf.gz" else f"{key}{ext}{comp}")
            p.write_bytes(blob)
            paths[(key, comp)] = str(p)
    return st, forms, paths


@pytest.mark.parametrize("form", ["fq", "mlfq", "fa"])
@pytest.mark.parametrize("comp", ["", ".gz", ".bgzf.gz"])
def test_files_dtable_and_descriptors(mix_files, form, comp):
    st, forms, paths = mix_files
    w = _check_files(st, [paths[(form, comp)]], [forms[form]], [form == "fa"], f"{form}{comp}")
    WORST["files"] = max(WORST.get("files", 0.0), w)


@pytest.mark.parametrize("comp", ["", ".gz", ".bgzf.gz"])
def test_fasta_after_four_line_fastq_keeps_descriptors(mix_files, comp):
    """a FASTA file behind a four-line file in one run: the FASTA chunks' holders get their names, and do not overwrite
    a good name taken from the four-line file with an empty one"""
    st, forms, paths = mix_files
    w = _check_files(st, [paths[("fq_head", comp)], paths[("fa_tail", comp)]], [forms["fq_head"], forms["fa_tail"]],
                     [False, True], f"fq+fa{comp}")
    WORST["files"] = max(WORST.get("files", 0.0), w)
