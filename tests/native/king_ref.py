"""The CPU statement of bed_king (king_ref.cpp, over bigsnpr_amd/csrc/king_step.hpp) for the tests and tools/probe_king.py:
built on first use with g++ -O2 -ffp-contract=off -fopenmp."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "king_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "king_step.hpp")]
SO = os.path.join(HERE, "libking_ref.so")
_lib = None

f64p, i32p, i8p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int8), C.POINTER(C.c_uint8)
COUNT_NAMES = ("NSNP", "HETHET", "IBS0", "HET1HOM2", "HET2HOM1")


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        cxx = os.environ.get("CXX", "g++")
        subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-fopenmp", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", CSRC,
                               SRC, "-o", SO + ".tmp"])
        os.replace(SO + ".tmp", SO)
    return SO


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        lib.king_table.restype = None
        lib.king_table.argtypes = [i8p, C.c_int64, C.c_int64, i32p, i32p, i32p, f64p]
        lib.king_filter.restype = None
        lib.king_filter.argtypes = [f64p, C.c_int64, C.c_double, u8p]
        _lib = lib
    return _lib


def table(G, thr=None):
    """the table of bed_king for the n x m codes G (0, 1, 2; 3 = missing): every pair i < j in the order (i, j), or those
    that pass `thr`"""
    G = np.ascontiguousarray(G, dtype=np.int8)
    n, m = G.shape
    k = n * (n - 1) // 2
    i1, i2 = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32)
    counts, kin = np.empty((k, 5), dtype=np.int32), np.empty(k)
    load().king_table(G.ctypes.data_as(i8p), n, m, i1.ctypes.data_as(i32p), i2.ctypes.data_as(i32p), counts.ctypes.data_as(i32p),
                      kin.ctypes.data_as(f64p))
    res = dict(I1=i1, I2=i2, KINSHIP=kin)
    for q, name in enumerate(COUNT_NAMES):
        res[name] = np.ascontiguousarray(counts[:, q])
    if thr is not None:
        keep = np.empty(k, dtype=np.uint8)
        load().king_filter(kin.ctypes.data_as(f64p), k, float(thr), keep.ctypes.data_as(u8p))
        res = {name: v[keep.astype(bool)] for name, v in res.items()}
    return res
