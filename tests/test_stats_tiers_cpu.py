"""The kernel table of tests/test_gpu_stats_tiers.py against the launch code: every kernel instantiation that
gs_launch_match, gs_launch_match_long, gs_launch_match_wide and gs_launch_match_huge can launch needs a row (and so a cell
of the matrix), and every row a kernel that exists.  The cells themselves are checked for what selects their kernels.
CPU only."""
import itertools
import os
import re

import pytest

import test_gpu_stats_tiers as tiers

SRC = os.path.join(tiers.CSRC, "gs_kernels.hip")
LAUNCHERS = ("gs_launch_match", "gs_launch_match_long", "gs_launch_match_wide", "gs_launch_match_huge")


def _body(src, head):
    """the text of the function whose definition starts with `head` (up to its matching closing brace)"""
    i = src.index(head)
    j = src.index("{", i)
    depth = 0
    for p in range(j, len(src)):
        depth += {"{": 1, "}": -1}.get(src[p], 0)
        if depth == 0:
            return src[j:p + 1]
    raise AssertionError(head)


def _template_params(src, kernel):
    """[(name, default or None)] of `template <...> __global__ ... void kernel(`"""
    m = re.search(r"template\s*<([^>]*)>\s*__global__[^;{]*?\bvoid\s+" + kernel + r"\s*\(", src)
    assert m, kernel
    out = []
    for p in m.group(1).split(","):
        decl, _, default = p.partition("=")
        out.append((decl.split()[-1], default.strip() or None))
    return out


def _canonical(src, kernel, args):
    params = _template_params(src, kernel)
    assert len(args) <= len(params), (kernel, args)
    full = args + [d for _, d in params[len(args):]]
    assert None not in full, (kernel, args)
    return "%s<%s>" % (kernel, ", ".join(full))


_INST = re.compile(r"(?:hipLaunchKernelGGL\s*\(\s*\(?|kern\s*=\s*)(gs_\w+_kernel)\s*<([^<>]*)>")


def launched(src=None):
    """{instantiation: launcher} of the four launch functions, gs_launch_match_t expanded"""
    src = src or open(SRC).read()
    out = {}
    t_body = _body(src, "static void gs_launch_match_t(")
    t_names = [n for _, n in (p.rsplit(None, 1) for p in re.search(r"template\s*<([^>]*)>\s*static void gs_launch_match_t",
                                                                     src).group(1).split(","))]
    for fn in LAUNCHERS:
        body = _body(src, 'extern "C" hipError_t %s(' % fn)
        for m in _INST.finditer(body):
            out[_canonical(src, m.group(1), [a.strip() for a in m.group(2).split(",")])] = fn
        for m in re.finditer(r"gs_launch_match_t\s*<([^<>]*)>", body):
            vals = dict(zip(t_names, [a.strip() for a in m.group(1).split(",")]))
            for k in _INST.finditer(t_body):
                args = [vals.get(a.strip(), a.strip()) for a in k.group(2).split(",")]
                out[_canonical(src, k.group(1), args)] = fn
    return out


def test_every_launched_kernel_has_a_row_and_every_row_a_kernel():
    got = launched()
    assert len(got) >= 50  # (24 + 14 + 8 + 8 today)
    missing = sorted(set(got) - set(tiers.KERNELS))
    assert not missing, f"kernel instantiations without a row (and a cell) in test_gpu_stats_tiers.KERNELS: {missing}"
    stale = sorted(set(tiers.KERNELS) - set(got))
    assert not stale, f"rows of test_gpu_stats_tiers.KERNELS that no launcher launches: {stale}"
    for inst, (fn, _) in tiers.KERNELS.items():
        assert got[inst] == fn, inst


def test_the_check_fails_for_a_new_instantiation_or_a_missing_row():
    src = open(SRC).read()
    base = launched(src)
    extra = src.replace("case 0: kern = gs_match_wide_kernel<false, 3, 0>; break;",
                        "case 0: kern = gs_match_wide_kernel<false, 3, 0>; break;\n        case 9: kern = gs_match_wide_kernel<false, 3, 27>; break;")
    assert extra != src
    assert set(launched(extra)) - set(tiers.KERNELS) == {"gs_match_wide_kernel<false, 3, 27>"}
    added = src.replace("hipLaunchKernelGGL((gs_match_huge_kernel<true, true>)",
                        "hipLaunchKernelGGL((gs_match_huge_kernel<true, true, 31>), dim3(1), dim3(1), 0, stream, *P);\n"
                        "            hipLaunchKernelGGL((gs_match_huge_kernel<true, true>)", 1)
    assert set(launched(added)) - set(base) == {"gs_match_huge_kernel<true, true, 31>"}
    row = next(iter(tiers.KERNELS))
    assert row in base and row not in {k: v for k, v in tiers.KERNELS.items() if k != row}


def _selects(c, d):
    """the kernel families a cell's batches reach, by the dispatch rules of gs_api.cpp launch_batch (a model of it, held to the
    table below)"""
    lds = "true" if c["nv"] <= d["GS_NV_LDS"] else "false"
    k31 = c["k"] == 31
    wide = c["paths"] > 64
    out = set()
    fam = c["family"]
    if c["layout"] == "part":
        out.add("gs_match_kernel<%s, true, 0, %s, false, 0>" % (lds, str(wide).lower()))
        if fam != "short":
            out.add("gs_match_long_kernel<%s, true, %s, false, 0>" % (lds, str(wide).lower()))
        return out
    striped = c["layout"] == "striped"
    ctx = 1 if c["ctx"] else 0
    if fam != "fixed250":
        if wide:
            out.add("gs_match_kernel<%s, false, 0, true, %s, 2>" % (lds, str(striped).lower()))
        else:
            out.add("gs_match_kernel<%s, false, %d, false, %s, %d>" % (lds, 31 if k31 else 0, str(striped).lower(), ctx))
    queues = {"short": [], "wide3": [3], "wide4": [4], "fixed250": [4], "long300": [5], "long1400": [5], "huge": [5, 6],
              "mixed": [3, 4, 5]}[fam]
    for q in queues:
        if q in (3, 4) and not wide and not striped:
            out.add("gs_match_wide_kernel<%s, %d, %d>" % (lds, q, 31 if k31 else 0))
        elif q in (3, 4, 5):
            kc = 31 if k31 and not wide and not striped else 0
            out.add("gs_match_long_kernel<%s, false, %s, %s, %d>" % (lds, str(wide).lower(), str(striped).lower(), kc))
        else:
            out.add("gs_match_huge_kernel<%s, %s, %d>" % (lds, str(striped).lower(), 31 if k31 and not striped else 0))
            out.add("gs_match_huge_finish_kernel<%s>" % lds)
    return out


def test_every_row_names_a_cell_that_selects_its_kernel():
    d = tiers.defines()
    for inst, (_, cell) in tiers.KERNELS.items():
        c = tiers.parse_cell(cell)
        assert inst in _selects(c, d), (inst, cell, sorted(_selects(c, d)))
    assert set(c for _, c in tiers.KERNELS.values()) <= set(tiers.cells())


def test_tier_limits_come_from_the_headers():
    d = tiers.defines()
    assert d["GS_NV_LDS"] < d["GS_NV_TREE_LDS"] < d["GS_STAT_REC_MAX_VALUES"] and d["GS_REDUCE_VALUES"] > 0
    for lim in ("GS_NV_LDS", "GS_NV_TREE_LDS", "GS_STAT_REC_MAX_VALUES"):  # each limit and the value above it is a tier
        assert d[lim] in tiers.TIERS and d[lim] + 1 in tiers.TIERS, lim
    rv = d["GS_REDUCE_VALUES"]
    assert {rv, rv + 1, 2 * rv + 1} <= set(tiers.TIERS)
    # fewer than 16 stat copies, and one copy, from the copy halving (copies * n_values * 96 > 64 MiB)
    assert any(16 * nv * 96 > (64 << 20) >= 8 * nv * 96 for nv in tiers.TIERS)
    assert any(2 * nv * 96 > (64 << 20) for nv in tiers.TIERS)
    for nv in tiers.TIERS:
        rows = tiers.target_rows(nv, d)
        assert nv - 1 in rows or nv == 1
        for p in range(min(-(-nv // rv), d["GS_STAT_REC_MAX_VALUES"] // rv)):
            assert p * rv in rows + [0] and min(p * rv + rv - 1, nv - 1) in rows + [nv - 1]


@pytest.mark.parametrize("axes", list(itertools.combinations(["k", "paths", "unique", "stat", "layout"], 2)))
def test_every_pair_of_axis_values_comes_up_in_the_sweep(axes):
    val = dict(k=lambda c: c["k"], paths=lambda c: c["paths"], unique=lambda c: c["unique"],
               stat=lambda c: (c["recs"], c["copies"]), layout=lambda c: c["layout"])
    cs = [tiers.parse_cell(c) for c in tiers.sweep_cells()]
    a, b = axes
    want = {(x, y) for x in {val[a](c) for c in cs} for y in {val[b](c) for c in cs}}
    assert want == {(val[a](c), val[b](c)) for c in cs}
    for nv in tiers.TIERS:  # and every tier meets every value of every axis, and every family
        mine = [c for c in cs if c["nv"] == nv]
        assert {val[a](c) for c in mine} == {val[a](c) for c in cs}
        assert {c["family"] for c in mine} == set(tiers.FAMILIES)
    assert len(cs) == len(tiers.TIERS) * len(tiers.FAMILIES)


def test_the_copy_halving_of_the_cells_is_the_library_s():
    """_preconditions halves the stat copies while copies * n_values * 96 > 64 MiB: the rule of gs_match_begin"""
    api = open(os.path.join(tiers.CSRC, "gs_api.cpp")).read()
    assert "while (copies > 1 && (size_t)copies * nv * 96 > ((size_t)64 << 20)) copies /= 2;" in api
    assert "run->use_stat_recs = nv <= GS_STAT_REC_MAX_VALUES;" in api
