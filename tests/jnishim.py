"""What tests/test_gpu_jni_dbchain.py and tests/test_jni_dbchain_cpu.py share: java/jni/gsgpu_jni.c compiled against the stand-in
jni.h with the functional JNIEnv of tests/native/jni_stub (as tests/test_gpu_jni.py does), and the "Java" objects a call takes --
Strings, String[], direct ByteBuffers with their capacities in elements, int[] and long[]."""
import ctypes as C
import os
import subprocess

import numpy as np

import genestrip_amd as ga
from conftest import ROOT
from genestrip_amd import host

PFX = "Java_org_metagene_genestrip_gpu_GsGpuNative_"
SHORT = b"gsgpu: buffer too small or missing"  # throw_short: IllegalArgumentException
J, I, Z = C.c_int64, C.c_int32, C.c_uint8      # jlong, jint, jboolean


class Shim:
    def __init__(self, path):
        L = self.L = C.CDLL(path)
        vp = C.c_void_p
        L.stub_env.restype = vp
        L.stub_string.restype, L.stub_string.argtypes = vp, [C.c_char_p]
        L.stub_buffer.restype, L.stub_buffer.argtypes = vp, [vp, C.c_int64]
        L.stub_long_array.restype, L.stub_long_array.argtypes = vp, [C.c_int32]
        L.stub_long_array_get.restype, L.stub_long_array_get.argtypes = C.c_int64, [vp, C.c_int32]
        L.stub_int_array.restype, L.stub_int_array.argtypes = vp, [C.c_int32]
        L.stub_int_array_set.argtypes = [vp, C.c_int32, C.c_int32]
        L.stub_object_array.restype, L.stub_object_array.argtypes = vp, [C.c_int32]
        L.stub_object_array_set.argtypes = [vp, C.c_int32, vp]
        L.stub_take_exception.restype = C.c_char_p
        self.env = vp(L.stub_env())
        self.keep = []  # a "direct buffer" is an address: the arrays behind them live as long as the shim

    def call(self, name, restype, *args, throws=False):
        """the native `name`; -> its result, or with throws=True the pending exception's message"""
        f = getattr(self.L, PFX + name)
        f.restype = restype
        got = f(self.env, None, *args)
        msg = self.L.stub_take_exception()
        if throws:
            assert msg is not None, name + " did not throw"
            return msg
        assert msg is None, (name, msg)
        return got

    def buf(self, a):
        """a numpy array as (direct ByteBuffer, capacity in elements); None as (null, 0)"""
        if a is None:
            return None, J(0)
        self.keep.append(a)
        return C.c_void_p(self.L.stub_buffer(a.ctypes.data_as(C.c_void_p), a.nbytes)), J(a.size)

    def text(self, data):
        a = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
        return (*self.buf(a), J(len(data)))

    def string(self, s):
        return None if s is None else C.c_void_p(self.L.stub_string(os.fsencode(s)))

    def strings(self, items):
        arr = self.L.stub_object_array(len(items))
        for i, s in enumerate(items):
            self.L.stub_object_array_set(arr, i, self.string(s))
        return C.c_void_p(arr)

    def longs(self, n):
        return C.c_void_p(self.L.stub_long_array(n))

    def ints(self, values):
        arr = self.L.stub_int_array(len(values))
        for i, v in enumerate(values):
            self.L.stub_int_array_set(arr, i, int(v))
        return C.c_void_p(arr)

    def get(self, arr, n):
        return [self.L.stub_long_array_get(arr, i) for i in range(n)]


def build(out):
    """java/jni/gsgpu_jni.c and the functional JNIEnv as one shared library at `out` -> Shim"""
    ga.lib()
    host.lib()
    cmd = ["gcc", "-shared", "-fPIC", "-Wall", "-I" + os.path.join(ROOT, "tests", "native", "jni_stub"), "-I" + os.path.join(ROOT, "include"), "-o", out,
           os.path.join(ROOT, "java", "jni", "gsgpu_jni.c"), os.path.join(ROOT, "tests", "native", "jni_stub", "jni_env.c"),
           "-L" + os.path.join(ROOT, "genestrip_amd"), "-lgshost", "-lgsgpu", "-Wl,-rpath," + os.path.join(ROOT, "genestrip_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return Shim(out)
