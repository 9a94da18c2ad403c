"""The CPU statement of snp_ancestry_summary / bed_ancestry (ancestry_ref.cpp, over bigsnpr_amd/csrc/qp_step.hpp with its
one-lane group) for the tests and tools/probe_ancestry.py: built on first use with g++ -O2 -ffp-contract=off -fopenmp."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "ancestry_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "qp_step.hpp")]
SO = os.path.join(HERE, "libancestry_ref.so")
_lib = None

f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
i64 = C.c_int64
REFUSALS = {1: "K < 1", 2: "K above the cap", 3: "D has no Cholesky factor"}


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
        lib.qp_max_k.restype = C.c_int
        lib.qp_iter_cap.restype = C.c_int
        lib.qp_iter_cap.argtypes = [C.c_int]
        lib.anc_slab_rows.restype = i64
        lib.anc_max_l.restype = C.c_int
        lib.qp_simplex.restype = C.c_int
        lib.qp_simplex.argtypes = [f64p, i64, f64p, i64, C.c_int, f64p, i32p, i64p]
        lib.anc_moments.restype = None
        lib.anc_moments.argtypes = [f64p, i64, f64p, i64, f64p, i64, i64, C.c_int, C.c_int, i64] + [f64p] * 7
        lib.ancestry_summary.restype = C.c_int
        lib.ancestry_summary.argtypes = [f64p, i64, i64, f64p, i64, f64p, i64, f64p, i64, C.c_int, C.c_int, f64p, C.c_int, f64p, f64p,
                                         f64p, i32p]
        lib.ancestry_rows.restype = C.c_int
        lib.ancestry_rows.argtypes = [f64p, i64, i64, i64, f64p, f64p, f64p, C.c_int, C.c_int, f64p, C.c_int, f64p, f64p, f64p, i32p]
        _lib = lib
    return _lib


class Refused(ValueError):
    pass


def _f(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _p(a):
    return None if a is None else a.ctypes.data_as(f64p)


def max_k():
    return load().qp_max_k()


def slab_rows():
    return int(load().anc_slab_rows())


def _checked(rc):
    if rc != 0:
        raise Refused(REFUSALS[rc])


def qp_simplex(D, d, sum_to_one=True):
    """d: K, or K x B (one problem per column).  dict(w: B x K, steps: B, n_failed)"""
    D = _f(D)
    d = _f(d)
    if d.ndim == 1:
        d = d[:, None]
    K, B = D.shape[0], d.shape[1]
    w = np.zeros((B, K), order="F")
    steps = np.zeros(B, dtype=np.int32)
    nf = C.c_int64(0)
    _checked(load().qp_simplex(_p(D), K, _p(d), B, int(bool(sum_to_one)), _p(w), steps.ctypes.data_as(i32p), C.byref(nf)))
    return dict(w=w, steps=steps, n_failed=nf.value)


def moments(P, X0, F=None):
    """dict(PtX0, PtF, G0, X0tF, csX0, csF, sqF) by plain loops"""
    P, X0 = _f(P), _f(X0)
    M, L = P.shape
    K = X0.shape[1]
    F = np.zeros((M, 0), order="F") if F is None else _f(F)
    if F.ndim == 1:
        F = _f(F[:, None])
    B = F.shape[1]
    out = dict(PtX0=np.zeros((L, K), order="F"), PtF=np.zeros((L, B), order="F"), G0=np.zeros((K, K), order="F"),
               X0tF=np.zeros((K, B), order="F"), csX0=np.zeros(K), csF=np.zeros(B), sqF=np.zeros(B))
    load().anc_moments(_p(P), max(M, 1), _p(X0), max(M, 1), _p(F), max(M, 1), M, L, K, B,
                       *[_p(out[k]) for k in ("PtX0", "PtF", "G0", "X0tF", "csX0", "csF", "sqF")])
    return out


def _results(B, K):
    return (np.zeros((B, K), order="F"), np.zeros((B, K), order="F"), np.zeros(B), np.zeros(B, dtype=np.int32))


def ancestry_summary(F, X0, P, correction, Dmat, sum_to_one=True):
    """F: M x B.  dict(w, cor_each: B x K; cor_pred, steps: B)"""
    F, X0, P, Dmat = _f(F), _f(X0), _f(P), _f(Dmat)
    if F.ndim == 1:
        F = _f(F[:, None])
    corr = np.ascontiguousarray(correction, dtype=np.float64)
    M, B = F.shape
    K, L = X0.shape[1], P.shape[1]
    w, ce, cp, steps = _results(B, K)
    _checked(load().ancestry_summary(_p(F), M, B, _p(X0), M, _p(P), M, _p(corr), M, L, K, _p(Dmat), int(bool(sum_to_one)), _p(w),
                                     _p(ce), _p(cp), steps.ctypes.data_as(i32p)))
    return dict(w=w, cor_each=ce, cor_pred=cp, steps=steps)


def ancestry_rows(G, X0, P, correction, Dmat, sum_to_one=True):
    """G: n x m allele counts (no missing value: the caller has replaced them).  As ancestry_summary, one problem per row."""
    G, X0, P, Dmat = _f(G), _f(X0), _f(P), _f(Dmat)
    corr = np.ascontiguousarray(correction, dtype=np.float64)
    n, m = G.shape
    K, L = X0.shape[1], P.shape[1]
    w, ce, cp, steps = _results(n, K)
    _checked(load().ancestry_rows(_p(G), n, n, m, _p(X0), _p(P), _p(corr), L, K, _p(Dmat), int(bool(sum_to_one)), _p(w), _p(ce),
                                  _p(cp), steps.ctypes.data_as(i32p)))
    return dict(w=w, cor_each=ce, cor_pred=cp, steps=steps)
