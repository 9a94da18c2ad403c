"""The CPU statement of big_spLinReg / big_spLogReg (plr_ref.cpp, over bigsnpr_amd/csrc/plr_step.hpp) for the tests and
tools/probe_plr.py: built on first use with g++ -O2 -ffp-contract=off (OpenMP over chains when the compiler has it).  It
takes the decoded values as a dense n x m matrix of doubles without missing values."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "plr_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "plr_step.hpp"), os.path.join(CSRC, "gibbs_step.hpp")]
SO = os.path.join(HERE, "libplr_ref.so")
_lib = None

i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
MESSAGES = ("", "No more improvement", "Too many variables", "Model saturated", "Complete path")


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        cxx = os.environ.get("CXX", "g++")
        base = [cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", CSRC, SRC, "-o", SO + ".tmp"]
        try:
            subprocess.check_call(base[:1] + ["-fopenmp"] + base[1:])
        except subprocess.CalledProcessError:
            subprocess.check_call(base)
        os.replace(SO + ".tmp", SO)
    return SO


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        lib.plr_ref_fit.restype = None
        lib.plr_ref_fit.argtypes = [f64p, C.c_int64, C.c_int64, f64p, f64p, C.c_int, f64p, i32p, C.c_int, f64p, C.c_int, i32p,
                                    f64p, C.c_int, C.c_int, C.c_int] + [f64p] * 5 + [i32p] * 6
        _lib = lib
    return _lib


def _p(a, t=f64p):
    return a.ctypes.data_as(t)


def fit(X, y, fold, K, alphas=(1.0,), covar=None, pf=None, family="linear", nlambda=200, lambda_min_ratio=None, nlam_min=50,
        n_abort=10, dfmax=50000, eps=1e-5, max_iter=1000, exact=True, reverse=False, nthreads=0):
    """dict of the raw outputs, chain c = a K + k in the last axis: intercept [C], beta [m + q, C], lambda / loss /
    loss_val / iter / nb_active [nlambda, C], n_done, best, status [C], turns [C] (the sweeps after l = 0: the turns of the
    device's host loop in which the chain is live)"""
    X = np.asfortranarray(X, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    n, m = X.shape
    y = np.ascontiguousarray(y, dtype=np.float64)
    cov = np.empty((n, 0), order="F") if covar is None else np.asfortranarray(covar, dtype=np.float64)
    q = cov.shape[1]
    pf = np.r_[np.ones(m), np.zeros(q)] if pf is None else np.ascontiguousarray(pf, dtype=np.float64)
    assert pf.size == m + q
    fold = np.ascontiguousarray(fold, dtype=np.int32)
    alphas = np.atleast_1d(np.asarray(alphas, dtype=np.float64))
    Cn = K * alphas.size
    if lambda_min_ratio is None:
        lambda_min_ratio = 1e-4 if n > m else 1e-3
    oi = np.array([0 if family == "linear" else 1, nlambda, nlam_min, n_abort, dfmax, max_iter], dtype=np.int32)
    od = np.array([eps, lambda_min_ratio], dtype=np.float64)
    out = dict(intercept=np.empty(Cn), beta=np.empty((m + q, Cn), order="F"))
    for k in ("lambda", "loss", "loss_val"):
        out[k] = np.empty((nlambda, Cn), order="F")
    for k in ("iter", "nb_active"):
        out[k] = np.empty((nlambda, Cn), dtype=np.int32, order="F")
    for k in ("n_done", "best", "status", "turns"):
        out[k] = np.empty(Cn, dtype=np.int32)
    load().plr_ref_fit(_p(X), n, m, _p(y), _p(cov) if q else None, q, _p(pf), _p(fold, i32p), int(K), _p(alphas), alphas.size,
                       _p(oi, i32p), _p(od), int(bool(exact)), int(bool(reverse)), int(nthreads), _p(out["intercept"]),
                       _p(out["beta"]), _p(out["lambda"]), _p(out["loss"]), _p(out["loss_val"]), _p(out["iter"], i32p),
                       _p(out["nb_active"], i32p), _p(out["n_done"], i32p), _p(out["best"], i32p), _p(out["status"], i32p),
                       _p(out["turns"], i32p))
    return out
