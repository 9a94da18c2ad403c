"""The host build of bigsnpr_amd/csrc/prodt_sparse.hpp (prodt_sparse_ref.cpp) for tests/test_prodt_sparse_cpu.py: built on
first use with g++ -O2."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "prodt_sparse_ref.cpp")
HDR = os.path.join(ROOT, "bigsnpr_amd", "csrc", "prodt_sparse.hpp")
SO = os.path.join(HERE, "libprodt_sparse_ref.so")
_lib = None

u32p, i8p = C.POINTER(C.c_uint32), C.POINTER(C.c_int8)


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        cxx = os.environ.get("CXX", "g++")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDR), SRC,
                               "-o", SO + ".tmp"])
        os.replace(SO + ".tmp", SO)
    return SO


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        lib.pts_decode.restype = None
        lib.pts_decode.argtypes = [u32p, C.c_int64, u32p, u32p]
        lib.pts_dot.restype = C.c_int64
        lib.pts_dot.argtypes = [C.c_uint32, i8p, i8p, C.POINTER(C.c_int)]
        _lib = lib
    return _lib


def decode(w):
    """values [n x 16] (variant order) and index fields [n x 16] of the dwords w"""
    w = np.ascontiguousarray(w, dtype=np.uint32).ravel()
    a, idx = np.empty(4 * w.size, dtype=np.uint32), np.empty(w.size, dtype=np.uint32)
    load().pts_decode(w.ctypes.data_as(u32p), w.size, a.ctypes.data_as(u32p), idx.ctypes.data_as(u32p))
    vals = a.view(np.uint8).reshape(w.size, 16)      # (little endian: byte i of dword r = value 4 r + i)
    fields = (idx[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3
    return vals, fields


def dot(w, dA, dB):
    """(sum, legal) of one lane group of the sparse instruction on dword w and the digits dA, dB [16] of its variants"""
    dA, dB = np.ascontiguousarray(dA, dtype=np.int8), np.ascontiguousarray(dB, dtype=np.int8)
    legal = C.c_int(0)
    s = load().pts_dot(int(w), dA.ctypes.data_as(i8p), dB.ctypes.data_as(i8p), C.byref(legal))
    return int(s), bool(legal.value)
