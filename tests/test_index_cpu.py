"""The index goal (gs_bloom_build_db, gs_bloom_get_info, gs_bloom_save / gs_bloom_load) without a GPU: the symbols exist and are
bound, bad arguments are refused before a device is touched, and the loader of the native index file refuses every defect of a
file written here from the layout include/gsgpu.h documents (on a machine without a GPU anything that got as far as the device
would answer GS_E_NODEVICE instead)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import genestrip_amd as ga
from genestrip_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gs_bloom_build_db", "gs_bloom_get_info", "gs_bloom_save", "gs_bloom_load")
INVALID, UNSUPPORTED, NODEVICE, IO = -1, -4, -6, -7
M64 = (1 << 64) - 1


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "gsgpu.h")).read()
    declared = set(re.findall(r"\b(gs_bloom_[a-z_0-9]+)\s*\(", header))
    assert declared == set(SYMBOLS) | {"gs_bloom_create", "gs_bloom_build", "gs_bloom_get", "gs_bloom_destroy"}
    L = ga.lib()
    for name in SYMBOLS:
        assert name in ga.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert ga.abi_version() == 3  # additive change
    for m in ("from_store", "load", "save", "info", "get", "build"):
        assert callable(getattr(ga.DeviceBloomFilter, m)), m
    assert callable(ga.requested_mask)


def test_info_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "gsgpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gs_bloom_info;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    ctype = {C.c_int32: "int32_t", C.c_int64: "int64_t", C.c_double: "double"}
    assert fields == [(n, ctype[t]) for n, t in binding.BloomInfo._fields_]
    assert C.sizeof(binding.BloomInfo) == 56


def _build_db(out=True, db=None, kind=ga.BLOOM_XOR, requested=True, expected=-1, fpp=1e-8):
    h = C.c_void_p()
    req = np.ones(4, np.uint8)
    n = C.c_int64(0)
    rc = ga.lib().gs_bloom_build_db(C.byref(h) if out else None, db, kind, req.ctypes.data_as(C.c_void_p) if requested else None,
                                    expected, fpp, C.byref(n))
    assert not h.value
    return rc


def test_build_db_refuses_bad_arguments_before_any_device():
    """there is no store without a device, so db is NULL throughout: the message tells which check answered"""
    err = lambda: ga.lib().gs_last_error().decode()
    assert _build_db(out=False) == INVALID and "out is NULL" in err()
    assert _build_db(db=None) == INVALID and "db is NULL" in err()
    assert _build_db(requested=False) == INVALID and "NULL" in err()
    for kind in (-1, 3):
        assert _build_db(kind=kind) == INVALID and "kind" in err()
    assert _build_db(expected=0) == INVALID and "expected_insertions" in err()
    for kind in (ga.BLOOM_XOR, ga.BLOOM_MURMUR):
        for fpp in (0.0, 1.0, -0.5, 2.0, float("nan")):
            assert _build_db(kind=kind, fpp=fpp) == INVALID and "fpp" in err(), (kind, fpp)
    assert _build_db(kind=ga.BLOOM_BLOCKED, fpp=0.0) == INVALID and "db is NULL" in err()  # fpp is ignored for a blocked filter


def test_the_other_calls_refuse_null_handles_and_paths(tmp_path):
    L = ga.lib()
    h = C.c_void_p()
    info = binding.BloomInfo()
    path = str(tmp_path / "x.gsindex").encode()
    assert L.gs_bloom_save(None, path) == INVALID
    assert L.gs_bloom_save(None, None) == INVALID
    assert L.gs_bloom_get_info(None, C.byref(info)) == INVALID
    assert L.gs_bloom_get_info(None, None) == INVALID
    assert L.gs_bloom_load(None, 0, path) == INVALID
    assert L.gs_bloom_load(C.byref(h), 0, None) == INVALID and not h.value
    assert L.gs_last_error()
    assert not os.path.exists(path)


# ---- the native index file, written from the layout the header documents
def checksum(payload):
    """the store file's checksum over the payload's 32-bit words: a = 1, b = 0; a += w, b += a; a ^ (b << 1) ^ (b >> 63)"""
    w = np.frombuffer(payload, dtype="<u4").astype(np.uint64)
    a_i = np.uint64(1) + np.cumsum(w, dtype=np.uint64)  # (uint64 arithmetic wraps mod 2^64)
    a = int(a_i[-1]) if len(w) else 1
    b = int(np.sum(a_i, dtype=np.uint64)) if len(w) else 0
    return (a ^ ((b << 1) & M64) ^ (b >> 63)) & M64


def index_file(kind=ga.BLOOM_XOR, k=31, bits=1000, n_hashes=3, n_words=None, expected=50, inserted=50, fpp=1e-3, magic=b"GSINDEX1",
               factors=None, words=None):
    if n_words is None:
        n_words = bits + 17 if kind == ga.BLOOM_BLOCKED else (bits + 63) // 64
    rng = np.random.default_rng(1)
    if factors is None:
        factors = rng.integers(-(1 << 62), 1 << 62, max(n_hashes, 0), dtype=np.int64)
    if words is None:
        words = rng.integers(0, 1 << 63, max(n_words, 0), dtype=np.uint64)
    payload = np.asarray(factors, "<i8").tobytes() + np.asarray(words, "<u8").tobytes()
    head = magic + struct.pack("<4i4qdQ", kind, k, n_hashes, 0, bits, n_words, expected, inserted, fpp, checksum(payload))
    assert len(head) == 72
    return head + payload


def _load(tmp_path, data, name="case.gsindex"):
    p = tmp_path / name
    p.write_bytes(data)
    h = C.c_void_p()
    rc = ga.lib().gs_bloom_load(C.byref(h), 0, str(p).encode())
    msg = ga.lib().gs_last_error().decode()
    if h.value:
        ga.lib().gs_bloom_destroy(h)
    return rc, msg, str(p)


def test_checksum_restatement():
    assert checksum(b"") == 1
    w = [3, 0xFFFFFFFF, 7]
    a, b = 1, 0
    for x in w:
        a = (a + x) & M64
        b = (b + a) & M64
    assert checksum(struct.pack("<3I", *w)) == (a ^ ((b << 1) & M64) ^ (b >> 63)) & M64


@pytest.mark.parametrize("kind", [ga.BLOOM_XOR, ga.BLOOM_MURMUR, ga.BLOOM_BLOCKED])
def test_a_sound_file_gets_as_far_as_the_device(tmp_path, kind):
    """the defect cases below are refused for their defect, not for the way this test writes files"""
    rc, msg, _ = _load(tmp_path, index_file(kind=kind, bits=300, n_hashes=1 if kind == ga.BLOOM_BLOCKED else 5))
    assert rc == (0 if ga.device_count() > 0 else NODEVICE), msg


DEFECTS = {
    "wrong magic": lambda: index_file(magic=b"GSINDEX0"),
    "truncated header": lambda: index_file()[:71],
    "empty file": lambda: b"",
    "truncated payload": lambda: index_file()[:-1],
    "payload cut at the words": lambda: index_file()[:72 + 3 * 8],
    "one byte too many": lambda: index_file() + b"\0",
    "n_hashes = 0": lambda: index_file(n_hashes=0),
    "n_hashes = 65": lambda: index_file(n_hashes=65),
    "unknown kind": lambda: index_file(kind=3),
    "n_words too small": lambda: index_file(bits=1000, n_words=15),
    "n_words too large": lambda: index_file(bits=1000, n_words=17),
    "blocked n_words": lambda: index_file(kind=ga.BLOOM_BLOCKED, bits=100, n_hashes=1, n_words=116),
    "blocked with two seeds": lambda: index_file(kind=ga.BLOOM_BLOCKED, bits=100, n_hashes=2),
    "bits = 0": lambda: index_file(bits=0, n_words=0),
    "negative n_words": lambda: index_file(bits=-64, n_words=-1),
    "bits above 2^37": lambda: index_file(bits=(1 << 37) + 1, n_words=3, words=np.zeros(3, np.uint64)),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_loader_refuses_a_defect_before_any_device(tmp_path, name):
    rc, msg, path = _load(tmp_path, DEFECTS[name]())
    assert rc == INVALID, (name, rc, msg)
    assert path in msg, msg


def test_loader_refuses_every_flipped_payload_bit_position_class(tmp_path):
    """a flipped bit in the factors, in the first and in the last word: a checksum defect"""
    good = index_file()
    for byte in (72, 72 + 3 * 8, len(good) - 1):
        bad = bytearray(good)
        bad[byte] ^= 0x10
        rc, msg, path = _load(tmp_path, bytes(bad))
        assert rc == INVALID and path in msg and "checksum" in msg, (byte, rc, msg)


def test_file_reader_under_sanitizers(tmp_path):
    """the reader and its checks (gs_indexfile.h) as a program of their own, built with the address and undefined-behaviour
    sanitizers: every defect above, the flipped bits and sound files of all kinds give the library's verdicts and no report"""
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-pthread", "-Wall"]
    exe = str(tmp_path / "indexfile_sanitize")
    b = subprocess.run(["g++", *flags, "-o", exe, os.path.join(ROOT, "tests", "native", "indexfile_sanitize.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    files = {name: make() for name, make in DEFECTS.items()}
    good = index_file()
    for byte in (72, 72 + 3 * 8, len(good) - 1):
        bad = bytearray(good)
        bad[byte] ^= 0x10
        files["flipped bit at %d" % byte] = bytes(bad)
    sound = {"sound xor": good, "sound blocked": index_file(kind=ga.BLOOM_BLOCKED, bits=300, n_hashes=1),
             "sound 64 hashes": index_file(kind=ga.BLOOM_MURMUR, bits=64 * 1000 + 1, n_hashes=64)}
    paths = []
    for i, data in enumerate(list(files.values()) + list(sound.values())):
        p = tmp_path / ("f%d.gsindex" % i)
        p.write_bytes(data)
        paths.append(str(p))
    paths.append(str(tmp_path / "missing.gsindex"))
    r = subprocess.run([exe, *paths], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(paths)
    verdicts = [int(ln.split()[0]) for ln in lines]
    assert verdicts == [1] * len(files) + [0] * len(sound) + [2], list(zip(verdicts, list(files) + list(sound)))
    for ln, p in zip(lines[:len(files)], paths):
        assert p in ln
    assert lines[len(files)].split()[:3] == ["0", "3", "16"]


def test_a_missing_file_is_an_io_error(tmp_path):
    h = C.c_void_p()
    p = str(tmp_path / "none.gsindex")
    assert ga.lib().gs_bloom_load(C.byref(h), 0, p.encode()) == IO and not h.value
    assert p in ga.lib().gs_last_error().decode()


def test_python_wrapper_checks_the_length_first():
    class Info:
        n_values = 7

    class Store:  # (h = None would be refused by the library: the wrapper must not get that far)
        info, h = Info(), None

    for bad in (np.ones(6, np.uint8), np.ones(8, bool), np.ones((7, 1), np.uint8)):
        with pytest.raises(ValueError):
            ga.DeviceBloomFilter.from_store(Store(), bad)


def test_requested_mask():
    taxids = ["1", "1279", "1280", "562"]
    assert ga.requested_mask(taxids, ["562", 1280]).tolist() == [0, 0, 1, 1]
    assert ga.requested_mask(taxids, []).tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        ga.requested_mask(taxids, ["9606"])
