"""The CPU statement of snp_fst and snp_MAX3 (popstat_ref.cpp, over bigsnpr_amd/csrc/popstat_step.hpp) for the tests and
tools/probe_popstat.py: built on first use with g++ -O2 -ffp-contract=off."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "popstat_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "popstat_step.hpp")]
SO = os.path.join(HERE, "libpopstat_ref.so")
_lib = None

f64p, i64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        cxx = os.environ.get("CXX", "g++")
        subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", CSRC, SRC,
                               "-o", SO + ".tmp"])
        os.replace(SO + ".tmp", SO)
    return SO


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        lib.popstat_af.restype = C.c_double
        lib.popstat_af.argtypes = [C.c_int64, C.c_int64, C.c_int64]
        lib.popstat_fst.restype = None
        lib.popstat_fst.argtypes = [f64p, f64p, C.c_int64, C.c_int64, C.c_double, f64p, f64p, i32p, f64p, f64p]
        lib.popstat_block_sum.restype = C.c_double
        lib.popstat_block_sum.argtypes = [f64p, C.c_int64]
        lib.popstat_max3.restype = None
        lib.popstat_max3.argtypes = [i64p, i64p, C.c_int64, f64p, C.c_int64, f64p]
        _lib = lib
    return _lib


def af(c1, c2, N):
    return float(load().popstat_af(int(c1), int(c2), int(N)))


def maf_from_counts(counts, size):
    """what bed_MAF makes of a 4 x m count table over `size` rows: (af, N), through the header's af_from_counts"""
    counts = np.asarray(counts, dtype=np.int64)
    N = size - counts[3]
    return np.array([af(c1, c2, n) for c1, c2, n in zip(counts[1], counts[2], N)]), N.astype(np.float64)


def fst(af_rm, N_rm, min_maf=0.0):
    """dict(a, abc, keep, fst, overall = (ratio, numerator, denominator)) for af, N of shape (r, m)"""
    a_ = np.ascontiguousarray(af_rm, dtype=np.float64)
    n_ = np.ascontiguousarray(N_rm, dtype=np.float64)
    r, m = a_.shape
    assert n_.shape == (r, m)
    a, abc, f = np.empty(m), np.empty(m), np.empty(m)
    keep = np.empty(m, dtype=np.int32)
    ov = np.empty(3)
    load().popstat_fst(a_.ctypes.data_as(f64p), n_.ctypes.data_as(f64p), r, m, float(min_maf), a.ctypes.data_as(f64p),
                       abc.ctypes.data_as(f64p), keep.ctypes.data_as(i32p), f.ctypes.data_as(f64p), ov.ctypes.data_as(f64p))
    return dict(a=a, abc=abc, keep=keep.astype(bool), fst=f, overall=ov)


def block_sum(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return float(load().popstat_block_sum(x.ctypes.data_as(f64p), x.size))


def max3(cases_3m, controls_3m, val=(0, 0.5, 1)):
    """score per variant from the 3 x m tables of the cases' and the controls' counts of 0, 1, 2"""
    ca = np.ascontiguousarray(np.asarray(cases_3m, dtype=np.int64).T)
    co = np.ascontiguousarray(np.asarray(controls_3m, dtype=np.int64).T)
    m = ca.shape[0]
    v = np.ascontiguousarray(np.atleast_1d(val), dtype=np.float64)
    out = np.empty(m)
    load().popstat_max3(ca.ctypes.data_as(i64p), co.ctypes.data_as(i64p), m, v.ctypes.data_as(f64p), v.size,
                        out.ctypes.data_as(f64p))
    return out
