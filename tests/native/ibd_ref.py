"""The CPU statement of bed_ibd (ibd_ref.cpp, over bigsnpr_amd/csrc/ibd_step.hpp) for the tests and tools/probe_ibd.py:
built on first use with g++ -O2 -ffp-contract=off -fopenmp."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "ibd_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "ibd_step.hpp")]
SO = os.path.join(HERE, "libibd_ref.so")
_lib = None

f64p, i32p, i64p, i8p, u8p = (C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int8),
                              C.POINTER(C.c_uint8))
IBS_NAMES = ("IBS0", "IBS1", "IBS2")
EST_NAMES = ("Z0", "Z1", "Z2", "PI_HAT", "DST")
BRANCHES = ("z0>1", "z1>1", "z2>1", "z0<0", "z1<0", "z2<0", "bounded")
LEAF = 256


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
        lib.ibd_terms.restype = None
        lib.ibd_terms.argtypes = [i64p, C.c_int64, f64p, u8p]
        lib.ibd_moments.restype = None
        lib.ibd_moments.argtypes = [i8p, C.c_int64, C.c_int64, u8p, f64p, i64p]
        lib.ibd_table.restype = None
        lib.ibd_table.argtypes = [i8p, C.c_int64, C.c_int64, f64p, i32p, i32p, i32p, f64p, i64p]
        lib.ibd_estimate.restype = None
        lib.ibd_estimate.argtypes = [i64p, C.c_int64, f64p, f64p]
        lib.ibd_filter.restype = None
        lib.ibd_filter.argtypes = [f64p, C.c_int64, C.c_double, u8p]
        _lib = lib
    return _lib


def terms(counts):
    """(a, used): the five terms of every variant (m x 5) from its counts n0, n1, n2 (m x 3) and whether it is used"""
    c = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1, 3)
    a, used = np.empty((c.shape[0], 5)), np.empty(c.shape[0], dtype=np.uint8)
    load().ibd_terms(c.ctypes.data_as(i64p), c.shape[0], a.ctypes.data_as(f64p), used.ctypes.data_as(u8p))
    return a, used.astype(bool)


def moments(G, freq=None):
    """(E, n_used) of the n x m codes G (0, 1, 2; 3 = missing) over the frequency samples `freq` (bool per row; None: all)"""
    G = np.ascontiguousarray(G, dtype=np.int8)
    n, m = G.shape
    f = np.ones(n, dtype=np.uint8) if freq is None else np.ascontiguousarray(np.asarray(freq).astype(bool), dtype=np.uint8)
    E, used = np.empty(5), C.c_int64(0)
    load().ibd_moments(G.ctypes.data_as(i8p), n, m, f.ctypes.data_as(u8p), E.ctypes.data_as(f64p), C.byref(used))
    return E, int(used.value)


def estimate(ibs, E):
    """the estimate of the header for rows of (IBS0, IBS1, IBS2): k x 5 (Z0, Z1, Z2, PI_HAT, DST)"""
    c = np.ascontiguousarray(ibs, dtype=np.int64).reshape(-1, 3)
    E = np.ascontiguousarray(E, dtype=np.float64)
    est = np.empty((c.shape[0], 5))
    load().ibd_estimate(c.ctypes.data_as(i64p), c.shape[0], E.ctypes.data_as(f64p), est.ctypes.data_as(f64p))
    return est


def table(G, freq=None, min_pi_hat=None):
    """the table of bed_ibd for the codes G: every pair i < j in the order (i, j), or those with PI_HAT >= min_pi_hat;
    plus E, n_used and `fired`, how often each branch of the estimate fired over ALL pairs (a dict over BRANCHES)"""
    G = np.ascontiguousarray(G, dtype=np.int8)
    n, m = G.shape
    E, n_used = moments(G, freq)
    k = n * (n - 1) // 2
    i1, i2 = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32)
    ibs, est, fired = np.empty((k, 3), dtype=np.int32), np.empty((k, 5)), np.zeros(len(BRANCHES), dtype=np.int64)
    load().ibd_table(G.ctypes.data_as(i8p), n, m, E.ctypes.data_as(f64p), i1.ctypes.data_as(i32p), i2.ctypes.data_as(i32p),
                     ibs.ctypes.data_as(i32p), est.ctypes.data_as(f64p), fired.ctypes.data_as(i64p))
    res = dict(I1=i1, I2=i2)
    for q, name in enumerate(IBS_NAMES):
        res[name] = np.ascontiguousarray(ibs[:, q])
    for q, name in enumerate(EST_NAMES):
        res[name] = np.ascontiguousarray(est[:, q])
    if min_pi_hat is not None:
        keep = np.empty(k, dtype=np.uint8)
        pi = res["PI_HAT"]
        load().ibd_filter(pi.ctypes.data_as(f64p), k, float(min_pi_hat), keep.ctypes.data_as(u8p))
        res = {name: v[keep.astype(bool)] for name, v in res.items()}
    res["E"], res["n_used"], res["fired"] = E, n_used, dict(zip(BRANCHES, fired.tolist()))
    return res
