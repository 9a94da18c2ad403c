"""The CPU statement of the exact Hardy-Weinberg test and the QC comparisons (hwe_ref.cpp, over
bigsnpr_amd/csrc/hwe_step.hpp) for the tests and tools/probe_qc.py: built on first use with g++ -O2 -ffp-contract=off
-fopenmp."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "hwe_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "hwe_step.hpp")]
SO = os.path.join(HERE, "libhwe_ref.so")
_lib = None

f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


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
        lib.hwe_ref_exact.restype = None
        lib.hwe_ref_exact.argtypes = [i32p, C.c_int64, C.c_int, f64p, i64p]
        lib.hwe_ref_walks.restype = None
        lib.hwe_ref_walks.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int, f64p]
        lib.hwe_ref_too_many_missing.restype = C.c_int
        lib.hwe_ref_too_many_missing.argtypes = [C.c_int64, C.c_int64, C.c_double]
        lib.hwe_ref_missing_rate.restype = C.c_double
        lib.hwe_ref_missing_rate.argtypes = [C.c_int64, C.c_int64]
        lib.hwe_ref_maf.restype = C.c_double
        lib.hwe_ref_maf.argtypes = [C.c_int64, C.c_int64, C.c_int64]
        lib.hwe_ref_maf_too_low.restype = C.c_int
        lib.hwe_ref_maf_too_low.argtypes = [C.c_double, C.c_double]
        lib.hwe_ref_rejected.restype = C.c_int
        lib.hwe_ref_rejected.argtypes = [C.c_double, C.c_double]
        _lib = lib
    return _lib


def exact(counts, midp=False, steps=False):
    """p per variant from the 3 x m table of (hom1, het, hom2); with steps=True also the number of terms formed"""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.int32).reshape(3, -1).T)
    m = c.shape[0]
    p = np.empty(m)
    st = np.empty(m, dtype=np.int64)
    load().hwe_ref_exact(c.ctypes.data_as(i32p), m, int(bool(midp)), p.ctypes.data_as(f64p), st.ctypes.data_as(i64p))
    return (p, st) if steps else p


def exact1(hom1, het, hom2, midp=False):
    return float(exact(np.array([[hom1], [het], [hom2]]), midp)[0])


def walks(hom1, het, hom2, midp=False):
    """(total_down, tail_down, total_up, tail_up) of one variant"""
    out = np.empty(4)
    load().hwe_ref_walks(int(hom1), int(het), int(hom2), int(bool(midp)), out.ctypes.data_as(f64p))
    return tuple(out)


def too_many_missing(na, of, rate):
    return bool(load().hwe_ref_too_many_missing(int(na), int(of), float(rate)))


def missing_rate(na, of):
    return float(load().hwe_ref_missing_rate(int(na), int(of)))


def maf(c0, c1, c2):
    return float(load().hwe_ref_maf(int(c0), int(c1), int(c2)))


def maf_too_low(maf_j, thr):
    return bool(load().hwe_ref_maf_too_low(float(maf_j), float(thr)))


def rejected(p, thr):
    return bool(load().hwe_ref_rejected(float(p), float(thr)))
