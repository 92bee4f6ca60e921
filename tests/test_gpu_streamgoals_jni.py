"""hostExtractFiles and hostFasta2Fastq of java/jni/gsgpu_jni.c through the stand-in JNIEnv (tests/native/jni_stub), driven as a JVM
would drive them; results must equal the two Java loops restated in tests/streamgoals.py."""
import ctypes as C
import gzip
import os
import subprocess

import pytest

import genestrip_amd as ga
import streamgoals as sg
from conftest import GOLDEN, ROOT
from genestrip_amd import host

pytestmark = pytest.mark.gpu

PFX = "Java_org_metagene_genestrip_gpu_GsGpuNative_"


@pytest.fixture(scope="module")
def jni(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jni") / "libgsjni_stream.so")
    ga.lib()
    host.lib()
    cmd = ["gcc", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(ROOT, "tests", "native", "jni_stub"), "-I" + os.path.join(ROOT, "include"), "-o", out,
           os.path.join(ROOT, "java", "jni", "gsgpu_jni.c"), os.path.join(ROOT, "tests", "native", "jni_stub", "jni_env.c"),
           "-L" + os.path.join(ROOT, "genestrip_amd"), "-lgshost", "-lgsgpu", "-Wl,-rpath," + os.path.join(ROOT, "genestrip_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(out)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    L.stub_env.restype = vp
    L.stub_string.restype, L.stub_string.argtypes = vp, [C.c_char_p]
    L.stub_long_array.restype, L.stub_long_array.argtypes = vp, [i32]
    L.stub_long_array_get.restype, L.stub_long_array_get.argtypes = i64, [vp, i32]
    L.stub_object_array.restype, L.stub_object_array.argtypes = vp, [i32]
    L.stub_object_array_set.argtypes = [vp, i32, vp]
    L.stub_take_exception.restype = C.c_char_p
    f = getattr(L, PFX + "hostExtractFiles")
    f.restype, f.argtypes = None, [vp, vp, i32, vp, i32, vp, vp, vp]
    f = getattr(L, PFX + "hostFasta2Fastq")
    f.restype, f.argtypes = i64, [vp, vp, i32, vp, vp]
    return L


def _strings(L, items):
    arr = L.stub_object_array(len(items))
    for i, s in enumerate(items):
        L.stub_object_array_set(arr, i, L.stub_string(str(s).encode()))
    return arr


def test_extract_and_fasta2fastq_through_the_jni_shim(jni, tmp_path):
    L = jni
    fq = b"".join(b"@lane%d:%d\n%s\n+\n%s\n" % (i % 3, i, b"ACGTT" * (1 + i % 20), b"F" * (5 * (1 + i % 20))) for i in range(3000))
    fa = open(os.path.join(GOLDEN, "fasta2fastq", "fasta2fastqtest.fasta"), "rb").read()
    p1, p2 = tmp_path / "a.fastq.gz", tmp_path / "b.fasta"
    p1.write_bytes(gzip.compress(fq, compresslevel=1))
    p2.write_bytes(fa)
    key = fa[1:4].decode()
    out = tmp_path / "x.fastq.gz"
    totals = L.stub_long_array(4)
    for k_, want in ((b"lane1:", sg.extract(fq, b"lane1:")), (key.encode(), sg.extract(fa, key.encode(), fasta=True))):
        getattr(L, PFX + "hostExtractFiles")(L.stub_env(), None, 0, L.stub_string(k_), 31, _strings(L, [p1, p2]), L.stub_string(str(out).encode()), totals)
        assert L.stub_take_exception() is None
        assert gzip.decompress(out.read_bytes()) == want[0] and want[1] > 0
        assert [L.stub_long_array_get(totals, i) for i in (0, 3)] == [3006, want[1]]
    out2 = tmp_path / "y.fastq"
    n = getattr(L, PFX + "hostFasta2Fastq")(L.stub_env(), None, 0, _strings(L, [p2, p2]), L.stub_string(str(out2).encode()))
    assert L.stub_take_exception() is None
    assert n == 12 and out2.read_bytes() == sg.fasta2fastq_files([fa, fa])
    # a failure surfaces as the RuntimeException's message
    getattr(L, PFX + "hostFasta2Fastq")(L.stub_env(), None, 0, _strings(L, [tmp_path / "missing.fasta"]), L.stub_string(str(out2).encode()))
    msg = L.stub_take_exception()
    assert msg is not None and b"missing.fasta" in msg
