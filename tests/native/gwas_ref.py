"""The CPU statement of big_univLinReg / big_univLogReg (gwas_ref.cpp, over bigsnpr_amd/csrc/irls_step.hpp) for the tests
and tools/probe_gwas.py: built on first use with g++ -O2 -ffp-contract=off (OpenMP over variants when the compiler has
it).  It takes the decoded genotypes as a dense n x m matrix of doubles, NaN = missing."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "gwas_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "irls_step.hpp"), os.path.join(CSRC, "gibbs_step.hpp")]
SO = os.path.join(HERE, "libgwas_ref.so")
_lib = None

i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)


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
        lib.gwas_logreg.restype = C.c_int
        lib.gwas_logreg.argtypes = [f64p, C.c_int64, C.c_int64, f64p, f64p, C.c_int, C.c_double, C.c_int, f64p, f64p, i32p,
                                    C.c_int]
        lib.gwas_linreg.restype = None
        lib.gwas_linreg.argtypes = [f64p, C.c_int64, C.c_int64, f64p, f64p, C.c_int, f64p, f64p, C.c_int]
        lib.gwas_sample_map.restype = None
        lib.gwas_sample_map.argtypes = [f64p, f64p, C.c_int64, f64p, f64p]
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(f64p)


def _dense(X):
    X = np.asfortranarray(X, dtype=np.float64)
    return X[:, None] if X.ndim == 1 else X


def _cov(covar, n):
    if covar is None:
        return np.empty((n, 0), order="F")
    c = np.asfortranarray(covar, dtype=np.float64)
    return np.asfortranarray(c[:, None]) if c.ndim == 1 else c


def logreg(X, y01, covar=None, tol=1e-8, maxiter=20, nthreads=0):
    """dict(estim, std_err, score, niter)"""
    X = _dense(X)
    n, m = X.shape
    y = np.ascontiguousarray(y01, dtype=np.float64)
    cov = _cov(covar, n)
    q = cov.shape[1]
    estim, se, niter = np.empty(m), np.empty(m), np.empty(m, dtype=np.int32)
    rc = load().gwas_logreg(_p(X), n, m, _p(y), _p(cov) if q else None, q, float(tol), int(maxiter), _p(estim), _p(se),
                            niter.ctypes.data_as(i32p), int(nthreads))
    if rc:
        raise ValueError("the covariates-only model is singular")
    return dict(estim=estim, std_err=se, score=estim / se, niter=niter)


def covar_basis(covar, n, thr_eigval=1e-4):
    u, d, _ = np.linalg.svd(np.column_stack([np.ones(n), _cov(covar, n)]), full_matrices=False)
    return np.asfortranarray(u[:, d / np.sqrt(n) > thr_eigval])


def linreg(X, y, covar=None, thr_eigval=1e-4, nthreads=0):
    X = _dense(X)
    n, m = X.shape
    y = np.ascontiguousarray(y, dtype=np.float64)
    U = covar_basis(covar, n, thr_eigval)
    K = U.shape[1]
    estim, se = np.empty(m), np.empty(m)
    load().gwas_linreg(_p(X), n, m, _p(y), _p(U), K, _p(estim), _p(se), int(nthreads))
    return dict(estim=estim, std_err=se, score=estim / se, df=n - K - 1)


def sample_map(eta, y):
    eta, y = np.ascontiguousarray(eta, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    w, wz = np.empty_like(eta), np.empty_like(eta)
    load().gwas_sample_map(_p(eta), _p(y), eta.size, _p(w), _p(wz))
    return w, wz
