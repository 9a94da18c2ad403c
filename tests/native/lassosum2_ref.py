"""The CPU statement of lassosum2 (lassosum2_ref.c) for the tests and tools/probe_lassosum2.py: built on first use with
-O2 -ffp-contract=off (OpenMP over grid points when the compiler has it), plus a short pure-Python transliteration
that the C statement is checked against."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lassosum2_ref.c")
SO = os.path.join(HERE, "liblassosum2_ref.so")
_lib = None

i64p, i32p, f64p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(SRC):
        cc = os.environ.get("CC", "gcc")
        base = [cc, "-O2", "-ffp-contract=off", "-std=c99", "-fPIC", "-shared", SRC, "-o", SO + ".tmp", "-lm"]
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
        lib.ls2_grid.restype = None
        lib.ls2_grid.argtypes = [i64p, i32p, f64p, C.c_int64, f64p, C.c_int64, f64p, f64p, f64p, C.c_int64, i64p,
                                 C.c_double, C.c_int, C.c_double, f64p, i32p, i64p, f64p, C.c_int]
        _lib = lib
    return _lib


def full_csc(A):
    """full columns of a scipy matrix (symmetric, given whole) with ascending rows"""
    from scipy import sparse
    A = sparse.csc_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)


def grid(p, i, x, m2, beta_hat, pf, lam, delta, ind_sub=None, dfmax=200e3, maxiter=1000, tol=1e-5, nthreads=0):
    """every grid point g of (lam[g], delta[g]); returns beta [m x G] (NaN columns where the reference returns NA),
    num_iter [G], non-zero-shift steps [G], seconds [G]"""
    L = load()
    p, i, x = (np.ascontiguousarray(a, dtype=t) for a, t in ((p, np.int64), (i, np.int32), (x, np.float64)))
    bh, pf = np.ascontiguousarray(beta_hat, dtype=np.float64), np.ascontiguousarray(pf, dtype=np.float64)
    lam, delta = np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(delta, dtype=np.float64)
    sub = None if ind_sub is None else np.ascontiguousarray(ind_sub, dtype=np.int64)
    m, G = bh.size, lam.size
    beta = np.empty((m, G), order="F")
    iters = np.zeros(G, dtype=np.int32)
    moves = np.zeros(G, dtype=np.int64)
    secs = np.zeros(G)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    L.ls2_grid(ptr(p, i64p), ptr(i, i32p), ptr(x, f64p), int(m2), ptr(bh, f64p), m, ptr(pf, f64p), ptr(lam, f64p),
               ptr(delta, f64p), G, ptr(sub, i64p), float(dfmax), int(maxiter), float(tol), ptr(beta, f64p),
               ptr(iters, i32p), ptr(moves, i64p), ptr(secs, f64p), int(nthreads))
    return beta, iters, moves, secs


def py_one(p, i, x, m2, beta_hat, lam_j, dpo_j, ind_sub, dfmax, maxiter, tol):
    """src/lassosum2.cpp:8-70 line by line in Python floats (IEEE doubles, every operation rounded)"""
    def soft(z, l1, d):
        if z > 0:
            num = z - l1
            return num / d if num > 0 else 0.0
        num = z + l1
        return num / d if num < 0 else 0.0

    m = len(beta_hat)
    curr = [0.0] * m
    dots = [0.0] * m2
    gap0 = 0.0
    for b in beta_hat:
        gap0 = gap0 + b * b
    gap0 = 2 * gap0
    k = 0
    while k < maxiter:
        conv, df, gap = True, 0.0, 0.0
        for j in range(m):
            j2 = j if ind_sub is None else int(ind_sub[j])
            u = float(beta_hat[j]) - (dots[j2] - curr[j])
            nb = soft(u, float(lam_j[j]), float(dpo_j[j]))
            if nb != 0:
                gap += nb * nb
                df += 1
            shift = nb - curr[j]
            if shift != 0:
                if conv and abs(shift) > tol:
                    conv = False
                curr[j] = nb
                for e in range(int(p[j2]), int(p[j2 + 1])):
                    r = int(i[e])
                    dots[r] = dots[r] + float(x[e]) * shift
        if gap > gap0:
            curr = [math.nan] * m
            break
        if conv or df > dfmax:
            break
        k += 1
    return np.array(curr), k + 1


def full_from_upper(p, i, x, m2):
    """full columns (ascending rows) of the symmetric matrix whose upper triangle with the diagonal is the CSC (p, i, x):
    as_SFBM's expansion, on the host; explicit zeros and NaN stay as stored"""
    p, i, x = np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(x, dtype=np.float64)
    col = np.repeat(np.arange(m2, dtype=np.int64), np.diff(p))
    off = i < col
    rows = np.concatenate([i, col[off]])
    cols = np.concatenate([col, i[off]])
    vals = np.concatenate([x, x[off]])
    order = np.lexsort((rows, cols))
    rows, cols, vals = rows[order], cols[order], vals[order]
    fp = np.zeros(m2 + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=m2), out=fp[1:])
    return fp, rows.astype(np.int32), vals
