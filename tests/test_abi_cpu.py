"""CPU-side checks of the drop-in boundary: libgsgpu.so loads, exports every symbol include/gsgpu.h declares,
and refuses to compute without a GPU (there is no CPU fallback in the product path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import genestrip_amd as ga
from conftest import ROOT


def test_library_loads_and_exports_every_declared_symbol():
    L = ga.lib()
    header = open(os.path.join(ROOT, "include", "gsgpu.h")).read()
    declared = set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", header))
    assert declared == set(ga.ABI_SYMBOLS), declared ^ set(ga.ABI_SYMBOLS)
    for name in declared:
        assert hasattr(L, name), name
    assert ga.abi_version() == 3
    assert L.gs_strerror(-6).decode() == "no usable gfx950 device"


def test_device_cache_trim_needs_no_device():
    """gs_device_cache_trim frees the device blocks that wait for the next run; with nothing waiting (no GPU here) it just returns"""
    assert ga.lib().gs_device_cache_trim() == 0


def test_host_layer_exports_every_declared_symbol():
    from genestrip_amd import host
    L = host.lib()
    header = open(os.path.join(ROOT, "include", "gshost.h")).read()
    declared = set(re.findall(r"\b(gs_(?:fastq|host)_[a-z_0-9]+)\s*\(", header))
    assert len(declared) >= 9
    for name in declared:
        assert hasattr(L, name), name


def test_integration_md_names_every_entry_point():
    """INTEGRATION.md maps each entry point of both headers to the reference interface it replaces (or says that there is
    none): by its full name, or as a `_suffix` inside a `gs_family_a / _b / _c` group"""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = set()
    for h in ("gsgpu.h", "gshost.h"):
        names |= set(re.findall(r"\b(gs_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", h)).read()))
    missing = [n for n in sorted(names) if n not in doc and ("_" + n.rsplit("_", 1)[1]) not in doc]
    assert not missing, missing


def test_header_enums_match_binding():
    header = open(os.path.join(ROOT, "include", "gsgpu.h")).read()
    cols = re.search(r"enum \{\s*GS_C_READS = 0,(.*?)GS_N_COLS", header, re.S).group(1)
    assert len(re.findall(r"GS_C_", cols)) + 1 == ga.N_COLS
    sums = re.search(r"enum \{ GS_S_READS = 0,(.*?)GS_N_SUMS", header, re.S).group(1)
    assert len(re.findall(r"GS_S_", sums)) + 1 == ga.N_SUMS


@pytest.mark.skipif(ga.device_count() > 0, reason="only meaningful without a GPU")
def test_fails_loudly_without_gpu():
    with pytest.raises(ga.GsError) as e:
        ga.DeviceKMerStore(2, [5], [0], 1)
    assert e.value.code == -6
    with pytest.raises(ga.GsError):
        ga.DeviceBloomFilter(ga.BLOOM_XOR, 64, [1], np.zeros(1, np.uint64))


def test_product_package_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "genestrip_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".c")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "gs_oracle" not in txt and "libgsoracle" not in txt, f


def test_launchers_and_parameter_blocks_are_declared_once():
    """gs_launch.h is the one place where a launcher or a kernel parameter block is declared: no Gs* struct is defined in two
    files, no translation unit of libgsgpu.so holds an extern "C" prototype of its own, every kernel is defined in the one unit of
    its family, and gs_api.cpp names its device allocations (gs_dev_alloc / gs_dev_free) instead of redefining hipMalloc / hipFree"""
    csrc = os.path.join(ROOT, "genestrip_amd", "csrc")
    src = {f: open(os.path.join(csrc, f), errors="replace").read() for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".cpp"))}
    where = {}
    for f, txt in src.items():
        for name in set(re.findall(r"\bstruct (Gs\w+) \{", txt)):
            where.setdefault(name, []).append(f)
    for name in ("GsExportParams", "GsFastqParams", "GsQualityParams", "GsUpdateParams"):
        assert where.get(name) == ["gs_launch.h"], (name, where.get(name))
    twice = {n: fs for n, fs in where.items() if len(fs) > 1}
    assert not twice, twice

    obj = re.search(r"^OBJ := (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1)
    units = {os.path.basename(o)[:-2] for o in obj.split()} | {"gs_devcache"}
    files = [f for f in src if f.endswith((".hip", ".cpp")) and f.rsplit(".", 1)[0] in units]
    assert len(files) == len(units) >= 13, (sorted(files), sorted(units))
    for f in files:
        protos = [" ".join(m.group(0).split()) for m in re.finditer(r'extern "C"[^;{]*;', src[f])]
        assert not protos, (f, protos)

    # one unit per kernel family: every gs_*_kernel is defined in one file, gs_kernels.hip is the match unit alone, and the units
    # split off from it share their wave helpers through gs_wave.h
    kernels = {}
    for f, txt in src.items():
        for name in re.findall(r"__global__[^;{]*?\bvoid (gs_\w+_kernel)\(", txt):
            kernels.setdefault(name, []).append(f)
    assert len(kernels) >= 25 and kernels["gs_match_kernel"] == ["gs_kernels.hip"], sorted(kernels)
    twice = {n: fs for n, fs in kernels.items() if len(fs) > 1}
    assert not twice, twice
    moved = ("gs_filter", "gs_encode", "gs_route", "gs_unroute", "gs_probe_keys", "gs_segments", "gs_unique", "gs_bitmap", "gs_clear_seen", "gs_rec_")
    stray = [n for n, fs in kernels.items() if fs == ["gs_kernels.hip"] and n.startswith(moved)]
    assert not stray, stray
    for f in ("gs_route.hip", "gs_segments.hip", "gs_seen.hip", "gs_filter.hip"):
        assert f in files and '#include "gs_wave.h"' in src[f], f

    api = src["gs_api.cpp"]
    assert not re.search(r"#\s*define\s+hip(Malloc|Free)\b", api)
    bare = re.findall(r"\bhip(?:Malloc|Free)\(", api)
    assert not bare, len(bare)
    assert "hipHostMalloc(" in api and "gs_dev_alloc(" in api and "gs_dev_free(" in api


def test_host_staging_timer_and_fence_are_written_once():
    """gs_api.cpp holds one exception fence (the GS_API_CATCH macro), one rebase of a host batch's offsets (the staging type's
    upload) and one read-out of a kernel timer's event pairs: plain text counts, so a pasted copy shows"""
    api = open(os.path.join(ROOT, "genestrip_amd", "csrc", "gs_api.cpp"), errors="replace").read()
    assert api.count("catch (const std::bad_alloc") == 1
    assert api.count("#define GS_API_CATCH") == 1 and api.index("#define GS_API_CATCH") < api.index("catch (const std::bad_alloc")
    assert api.count("offsets[i] - offsets[0]") == 1
    assert api.count("hipEventElapsedTime(&ms, p.first, p.second)") == 1


def test_synth_reads_deterministic_and_shaped():
    from genestrip_amd import synth
    db = synth.SynthDB(k=31, genera=2, species_per_genus=2, genome_len=5000, seed=7)
    assert np.all(np.diff(db.kmers) > 0) and db.n_values == 7
    seq, off = synth.reads_host(db.genomes, 1000, read_len=150, seed=3)
    seq2, _ = synth.reads_host(db.genomes, 400, read_len=150, seed=3, first=600)
    assert np.array_equal(seq[600 * 150:], seq2)
    assert set(np.unique(seq).tolist()) <= set(b"ACGTN")
    assert off[-1] == 150000
