"""One checker for a whole match result (integer table, per-read outputs, double table, max hit counts) against the CPU
oracle.  A helper module of the suite, not a test file.

The integer table and the per-read outputs are compared bit for bit.  The double table (GS_D_*) is a sum of non-negative
float64 terms whose order of summation is the device's business, so each cell is compared with the exact sum S of the
terms the oracle says belong to it: the terms are formed as FastqKMerMatcher forms them (t = tax_err / max, t * t, and the
same for class_err), sorted by row and added with math.fsum (correctly rounded).  For non-negative terms any order of
summation lies within (n - 1) * 2^-53 * S of S (n = terms of the cell); the bound used is (n + 3) * 2^-53 * S, the + 3
for how a device forms a term.  A cell without terms must be exactly 0.0.
"""
import gzip
import math

import numpy as np

from oracle import gs_oracle as orc

EPS = 2.0 ** -53
D_COLS = ("err sum", "err sq sum", "class err sum", "class err sq sum")


def dtable_reference(terms, n_values):
    """(S float64[n_values, 4], n int64[n_values]) of the per-read terms (oracle MatchRun.submit_terms, any number of batches
    concatenated)"""
    terms = np.asarray(terms, dtype=np.int64).reshape(-1, orc.N_TERMS)
    terms = terms[terms[:, orc.T_CN] >= 0]
    terms = terms[np.argsort(terms[:, orc.T_CN], kind="stable")]
    cn = terms[:, orc.T_CN]
    assert cn.size == 0 or cn[-1] < n_values
    mx = terms[:, orc.T_MAX].astype(np.float64)
    t = terms[:, orc.T_TAX_ERR].astype(np.float64) / mx
    c = terms[:, orc.T_CLASS_ERR].astype(np.float64) / mx
    cols = (t, t * t, c, c * c)
    S = np.zeros((n_values, 4), dtype=np.float64)
    n = np.bincount(cn, minlength=n_values).astype(np.int64)
    bounds = np.concatenate([[0], np.cumsum(n)])
    for v in np.flatnonzero(n):
        lo, hi = int(bounds[v]), int(bounds[v + 1])
        for j in range(4):
            S[v, j] = math.fsum(cols[j][lo:hi].tolist())
    return S, n


def check_dtable(terms, n_values, dtable, what="dtable", ref=None):
    """asserts every cell of `dtable` is within (n + 3) * 2^-53 * S of the exact sum; returns the largest
    |g - S| / ((n + 3) * 2^-53 * S) over the cells with a non-zero sum (0.0 if there are none)"""
    S, n = dtable_reference(terms, n_values) if ref is None else ref
    g = np.asarray(dtable, dtype=np.float64)
    assert g.shape == (n_values, 4), (what, g.shape)
    assert np.all(np.isfinite(g)), f"{what}: non-finite cells at {np.argwhere(~np.isfinite(g))[:6].tolist()}"
    empty = S == 0.0  # no terms, or only zero terms: the sum is exact
    bad = np.argwhere(empty & (g != 0.0))
    assert bad.size == 0, f"{what}: cell (vi, col) {bad[0].tolist()} should be 0.0 (terms {int(n[bad[0][0]])}), is {g[tuple(bad[0])]!r}"
    tol = (n[:, None] + 3).astype(np.float64) * EPS * S
    err = np.abs(g - S)
    over = np.argwhere(~empty & (err > tol))
    if over.size:
        v, j = over[0].tolist()
        raise AssertionError(f"{what}: {len(over)} cells outside the bound, first (vi {v}, {D_COLS[j]}): {g[v, j]!r} vs exact "
                             f"{S[v, j]!r} over {int(n[v])} terms (|g - S| = {err[v, j]:.3e}, bound {tol[v, j]:.3e})")
    ratio = np.where(empty, 0.0, err / np.where(empty, 1.0, tol))
    return float(ratio.max()) if ratio.size else 0.0


def check_table(otable, gtable, what="table"):
    """integer table bit-exact in every column (the unique and the max-contig-read columns included)"""
    assert otable.shape == gtable.shape, (what, otable.shape, gtable.shape)
    bad = np.argwhere(otable != gtable)
    assert bad.size == 0, (f"{what} differs at {len(bad)} cells, first (vi, col) {bad[:6].tolist()}: oracle "
                           f"{otable[tuple(bad[0])]} device {gtable[tuple(bad[0])]}")


def check_match(o, g, what="match", ref=None):
    """o: dict(table, terms, [class_vi, flags, dtable, max_counts]) of the oracle; g: dict(table, dtable, [class_vi, flags,
    max_counts]) of the device.  Per-read outputs and max counts are compared when both sides have them; the oracle's own
    dtable, when given, is held to the same bound (which tests the checker).  ref: dtable_reference(o["terms"]) if already
    at hand.  Returns the worst dtable ratio."""
    check_table(o["table"], g["table"], what + ": table")
    for key in ("class_vi", "flags"):
        if o.get(key) is not None and g.get(key) is not None:
            a, b = np.asarray(o[key]), np.asarray(g[key])
            assert a.shape == b.shape, (what, key, a.shape, b.shape)
            assert np.array_equal(a, b), f"{what}: {key} differs at reads {np.flatnonzero(a != b)[:10].tolist()}"
    if o.get("max_counts") is not None and g.get("max_counts") is not None:
        bad = np.argwhere(o["max_counts"] != g["max_counts"])
        assert bad.size == 0, f"{what}: max_counts differ at (row, j) {bad[:6].tolist()}"
    nv = o["table"].shape[0]
    ref = dtable_reference(o["terms"], nv) if ref is None else ref
    # the counted reads of each row are the READS column: the terms belong to the rows they claim to
    assert np.array_equal(ref[1], o["table"][:, orc.C_READS]), f"{what}: oracle terms do not match its READS column"
    if o.get("dtable") is not None:
        check_dtable(o["terms"], nv, o["dtable"], what + " (oracle dtable)", ref=ref)
    return check_dtable(o["terms"], nv, g["dtable"], what, ref=ref)


def sum_dtables(parts):
    """the double tables of a result split over several runs (partition ranks, shards) added cell by cell in float64.
    Every part holds sums of the same non-negative terms, so the total is one more summation tree over them: it stays
    within (n - 1) * 2^-53 * S of the exact sum, and adding 0.0 is exact, so check_dtable's bound (n + 3) * 2^-53 * S
    holds for the total unchanged -- a term left out of every part, or counted in two, still fails it."""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    out = np.zeros_like(parts[0])
    for p in parts:
        assert p.shape == out.shape, (p.shape, out.shape)
        out = out + p
    return out


ADD_COLS = [orc.C_READS, 1, 2, orc.C_UNIQUE_KMERS, 4, 5, 7, 8]  # the additive columns of the integer table


def merge_tables(tables):
    """the integer tables of runs over disjoint shards of the reads (DB-partitioned ranks: the unique counts of the partitions are
    disjoint too) as one run gives it: additive columns added, the longest contig and its read number from the run that holds
    the longest one (on ties the lowest read number)"""
    out = np.zeros_like(tables[0])
    for c in ADD_COLS:
        out[:, c] = sum(t[:, c] for t in tables)
    uq = np.stack([t[:, orc.C_UNIQUE_KMERS] for t in tables])
    out[:, orc.C_UNIQUE_KMERS] = np.where(np.all(uq == -1, axis=0), -1, out[:, orc.C_UNIQUE_KMERS])  # (-1: not counted)
    for v in range(out.shape[0]):
        best = (0, -1)
        for t in tables:
            if t[v, 6] > best[0] or (t[v, 6] == best[0] and t[v, 6] > 0 and t[v, 9] < best[1]):
                best = (int(t[v, 6]), int(t[v, 9]))
        out[v, 6], out[v, 9] = best
    return out


def check_match_parts(o, parts, what="match", ref=None):
    """check_match of a result split over runs: parts = the device results (dict(table, dtable, [class_vi, flags])) of each
    run, in read order; tables merged (merge_tables), dtables added (sum_dtables), per-read outputs concatenated"""
    g = dict(table=merge_tables([p["table"] for p in parts]), dtable=sum_dtables([p["dtable"] for p in parts]))
    for key in ("class_vi", "flags"):
        if all(p.get(key) is not None for p in parts):
            g[key] = np.concatenate([np.asarray(p[key]) for p in parts])
    return check_match(o, g, what, ref=ref)


def _file_bytes(path):
    data = open(path, "rb").read()
    return gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data  # (gzip and BGZF: members back to back)


def oracle_files(odb, paths, threads=8, first_read_no=0, max_counts=False, **cfg):
    """the oracle side of a file-level test: the records of `paths` (FASTQ, multi-line FASTQ or FASTA -- a file whose first byte
    is '>' --, plain, gzip or BGZF) through one oracle run, in file order, read numbers running on over the files from
    first_read_no.  Returns dict(table, dtable, terms, class_vi, flags, reads, kmers, bps[, max_counts]) for check_match."""
    run = orc.MatchRun(odb, **cfg)
    cvs, fls, terms = [], [], []
    nr, nk, nb = 0, 0, 0
    for path in paths:
        data = _file_bytes(path)
        p = orc.parse_fastq(data, fasta=data[:1] == b">", k=odb.k)
        seq = p["seq"] if len(p["seq"]) else np.zeros(1, dtype=np.uint8)
        cv, fl, te = run.submit_terms(seq, p["seq_off"], first_read_no + nr, threads=threads)
        cvs.append(cv)
        fls.append(fl)
        terms.append(te)
        nr, nk, nb = nr + int(p["n_reads"]), nk + int(p["total_kmers"]), nb + int(p["total_bps"])
    t, d = run.finish()
    o = dict(table=t, dtable=d, class_vi=np.concatenate(cvs) if cvs else np.zeros(0, np.int32),
             flags=np.concatenate(fls) if fls else np.zeros(0, np.uint8),
             terms=np.concatenate(terms) if terms else np.zeros((0, orc.N_TERMS), np.int32), reads=nr, kmers=nk, bps=nb)
    if max_counts:
        o["max_counts"] = run.max_counts()
    run.close()
    return o


def oracle_batch(odb, seq, offsets, first_read_no=0, threads=8, max_counts=False, **cfg):
    """one oracle run over one batch of reads: dict(table, dtable, terms, class_vi, flags[, max_counts]) for check_match"""
    seq = np.asarray(seq, dtype=np.uint8)
    run = orc.MatchRun(odb, **cfg)
    cv, fl, terms = run.submit_terms(seq if len(seq) else np.zeros(1, dtype=np.uint8), offsets, first_read_no, threads=threads)
    t, d = run.finish()
    o = dict(table=t, dtable=d, class_vi=cv, flags=fl, terms=terms)
    if max_counts:
        o["max_counts"] = run.max_counts()
    run.close()
    return o


def check_dtables_agree(a, b, n, what="dtables"):
    """two device double tables over the same reads (summed in different orders, e.g. one batch against two): each cell is
    within (n + 3) * 2^-53 * S of the same exact sum S, so they differ by at most 2 (n + 3) * 2^-53 * max(a, b); n = counted reads
    per row (the READS column).  Cells of rows without counted reads must both be 0.0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    n = np.asarray(n, dtype=np.float64)[:, None]
    tol = 2.0 * (n + 3.0) * EPS * np.maximum(a, b)
    bad = np.argwhere(np.abs(a - b) > tol)
    assert bad.size == 0, f"{what}: {len(bad)} cells disagree, first (vi, col) {bad[0].tolist()}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"
