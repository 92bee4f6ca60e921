"""One checker for a whole match result (integer table, per-read outputs, double table, max hit counts) against the CPU
oracle.  A helper module of the suite, not a test file.

The integer table and the per-read outputs are compared bit for bit.  The double table (GS_D_*) is a sum of non-negative
float64 terms whose order of summation is the device's business, so each cell is compared with the exact sum S of the
terms the oracle says belong to it: the terms are formed as FastqKMerMatcher forms them (t = tax_err / max, t * t, and the
same for class_err), sorted by row and added with math.fsum (correctly rounded).  For non-negative terms any order of
summation lies within (n - 1) * 2^-53 * S of S (n = terms of the cell); the bound used is (n + 3) * 2^-53 * S, the + 3
for how a device forms a term.  A cell without terms must be exactly 0.0.
"""
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
