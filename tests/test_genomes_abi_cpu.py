"""The genomes stage (gs_genomes_*: genome FASTA text to build regions) without a GPU: the symbols are declared, exported and
bound, and every NULL or negative argument is refused with GS_E_INVALID before a device is touched (on a machine without a GPU
anything that got as far as the device would answer GS_E_NODEVICE instead)."""
import ctypes as C
import os
import re

import numpy as np

import genestrip_amd as ga

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gs_genomes_create", "gs_genomes_scan", "gs_genomes_headers", "gs_genomes_gather", "gs_genomes_regions",
           "gs_genomes_kernel_time", "gs_genomes_destroy")
INVALID = -1


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gsgpu.h")).read()
    declared = set(re.findall(r"\b(gs_genomes_[a-z_0-9]+)\s*\(", header))
    assert declared == set(SYMBOLS)
    L = ga.lib()
    for name in SYMBOLS:
        assert name in ga.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert ga.abi_version() == int(re.search(r"#define GS_ABI_VERSION (\d+)", header).group(1))
    for m in ("scan", "headers", "gather", "regions", "kernel_time", "close"):
        assert callable(getattr(ga.DeviceGenomes, m)), m


def test_the_kernels_are_one_unit_of_the_library():
    csrc = os.path.join(ROOT, "genestrip_amd", "csrc")
    assert "build/gs_genomes.o" in re.search(r"^OBJ := (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    launch = open(os.path.join(csrc, "gs_launch.h")).read()
    unit = open(os.path.join(csrc, "gs_genomes.hip")).read()
    defined = set(re.findall(r'extern "C" hipError_t (gs_launch_genomes_\w+)\(', unit))
    assert len(defined) == 5 and all(re.search(r"\b%s\(" % n, launch) for n in defined), defined
    assert "struct GsGenomesParams {" in open(os.path.join(csrc, "gs_params.h")).read()


def test_null_and_negative_arguments_are_refused_before_any_device():
    L = ga.lib()
    err = lambda: L.gs_last_error().decode()
    h = C.c_void_p()
    out = [C.c_int64(7) for _ in range(4)]
    refs = [C.byref(o) for o in out]
    text = np.frombuffer(b">a\nAC\n", dtype=np.uint8)
    tp = text.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(8)  # never dereferenced: every call below fails on another argument first

    assert L.gs_genomes_create(None, 0) == INVALID and "out is NULL" in err()
    assert L.gs_genomes_create(C.byref(h), -1) == INVALID and "device" in err()
    assert not h.value

    assert L.gs_genomes_scan(None, tp, len(text), ga.MEM_HOST, 1, *refs) == INVALID and "genomes is NULL" in err()
    assert L.gs_genomes_scan(fake, None, 6, ga.MEM_HOST, 1, *refs) == INVALID and "text" in err()
    assert L.gs_genomes_scan(fake, tp, -1, ga.MEM_HOST, 1, *refs) == INVALID and "negative" in err()
    for mem in (-1, 2, 3):
        assert L.gs_genomes_scan(fake, tp, len(text), mem, 1, *refs) == INVALID and "mem" in err()
    for i in range(4):
        args = list(refs)
        args[i] = None
        assert L.gs_genomes_scan(fake, tp, len(text), ga.MEM_HOST, 1, *args) == INVALID and "output" in err(), i

    off = np.zeros(4, dtype=np.uint64)
    hdr = np.zeros(16, dtype=np.uint8)
    assert L.gs_genomes_headers(None, hdr.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p)) == INVALID
    assert L.gs_genomes_headers(fake, hdr.ctypes.data_as(C.c_void_p), None) == INVALID

    n = C.c_int64(0)
    assert L.gs_genomes_gather(None, None, C.byref(n), C.byref(n)) == INVALID
    assert L.gs_genomes_gather(fake, None, None, C.byref(n)) == INVALID
    assert L.gs_genomes_gather(fake, None, C.byref(n), None) == INVALID

    p = C.c_void_p()
    assert L.gs_genomes_regions(None, C.byref(p), C.byref(p)) == INVALID
    assert L.gs_genomes_regions(fake, None, C.byref(p)) == INVALID
    assert L.gs_genomes_regions(fake, C.byref(p), None) == INVALID

    d = C.c_double(0)
    assert L.gs_genomes_kernel_time(None, C.byref(d), C.byref(d)) == INVALID
    assert L.gs_genomes_kernel_time(fake, None, C.byref(d)) == INVALID
    assert L.gs_genomes_kernel_time(fake, C.byref(d), None) == INVALID

    assert L.gs_genomes_destroy(None) == 0
