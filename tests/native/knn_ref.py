"""The CPU statement of knn_parallel / prob_dist / LOF (knn_ref.cpp, over bigsnpr_amd/csrc/knn_step.hpp and knn_plan.hpp)
for the tests and tools/probe_knn.py: built on first use with g++ -O2 -ffp-contract=off -fopenmp."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "knn_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "knn_step.hpp"), os.path.join(CSRC, "knn_plan.hpp")]
SO = os.path.join(HERE, "libknn_ref.so")
_lib = None

f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
i64 = C.c_int64


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
        lib.knn_table.restype = None
        lib.knn_table.argtypes = [f64p, i64, i64, f64p, i64, i64, C.c_int, C.c_int, i64, i64, i32p, f64p, f64p]
        lib.knn_prob_dist.restype = None
        lib.knn_prob_dist.argtypes = [f64p, i32p, i64, C.c_int, f64p, f64p]
        lib.knn_lof.restype = None
        lib.knn_lof.argtypes = [f64p, i32p, i64, i32p, C.c_int, f64p]
        lib.knn_plan.restype = None
        lib.knn_plan.argtypes = [i64, i64, C.c_int, C.c_int, i64, i64p, i64p, i64]
        lib.knn_partial_cap.restype = i64
        lib.knn_min_slab_points.restype = i64
        lib.knn_padded_p.restype = C.c_int
        lib.knn_padded_p.argtypes = [C.c_int]
        _lib = lib
    return _lib


def _f(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def padded_rows(a, ld):
    """a as the top rows of a column-major matrix of ld rows, the rows below them NaN (ld=None: a itself, column-major)"""
    a = _f(a)
    if ld is None:
        return a
    assert ld >= a.shape[0]
    out = np.full((ld, a.shape[1]), np.nan, order="F")
    out[:a.shape[0]] = a
    return out


def knn(data, query=None, k=1, rows=None, ld=None, ldq=None):
    """nn_idx (int32, 0-based), nn_d2, nn_dists: nq x k.  query=None: self mode.  rows=(q0, q1): those queries only (the
    other rows of the result are not filled).  ld / ldq: hand the matrices over as the top rows of larger ones (leading
    dimensions above the row counts; the rows below hold NaN)"""
    data = _f(data)
    n, p = data.shape
    q = None if query is None else _f(query)
    nq = n if q is None else q.shape[0]
    data = padded_rows(data, ld)
    q = None if q is None else padded_rows(q, ldq)
    q0, q1 = (0, nq) if rows is None else rows
    idx = np.zeros((nq, k), dtype=np.int32, order="F")
    d2, dist = np.zeros((nq, k), order="F"), np.zeros((nq, k), order="F")
    load().knn_table(data.ctypes.data_as(f64p), n, data.shape[0], None if q is None else q.ctypes.data_as(f64p), nq,
                     nq if q is None else q.shape[0], p, k, q0, q1, idx.ctypes.data_as(i32p), d2.ctypes.data_as(f64p),
                     dist.ctypes.data_as(f64p))
    return dict(nn_idx=idx, nn_d2=d2, nn_dists=dist)


def prob_dist(U, kNN=5):
    t = knn(U, None, kNN)
    n = t["nn_idx"].shape[0]
    ds, dn = np.empty(n), np.empty(n)
    load().knn_prob_dist(t["nn_d2"].ctypes.data_as(f64p), t["nn_idx"].ctypes.data_as(i32p), n, kNN, ds.ctypes.data_as(f64p),
                         dn.ctypes.data_as(f64p))
    return dict(dist_self=ds, dist_nn=dn)


def lof(U, seq_k=(4, 10, 30)):
    """the n x len(seq_k) matrix of local outlier factors"""
    seq = np.ascontiguousarray(seq_k, dtype=np.int32)
    t = knn(U, None, int(seq.max()))
    n = t["nn_idx"].shape[0]
    out = np.empty((n, seq.size), order="F")
    load().knn_lof(t["nn_dists"].ctypes.data_as(f64p), t["nn_idx"].ctypes.data_as(i32p), n, seq.ctypes.data_as(i32p), seq.size,
                   out.ctypes.data_as(f64p))
    return out


def plan(n, nq, k, ncu=256, forced=0):
    out = np.zeros(4, dtype=np.int64)
    L = load()
    L.knn_plan(n, nq, k, ncu, forced, out.ctypes.data_as(i64p), None, 0)
    lo = np.zeros(int(out[2]) + 1, dtype=np.int64)
    L.knn_plan(n, nq, k, ncu, forced, out.ctypes.data_as(i64p), lo.ctypes.data_as(i64p), lo.size)
    return dict(qb=int(out[0]), nqb=int(out[1]), S=int(out[2]), partial_bytes=int(out[3]), lo=lo)
