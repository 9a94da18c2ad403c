"""The CPU comparator of tools/probe_sfbm.py (sfbm_ref.c): the sparse symmetric product and the column sums of squares with
OpenMP over the columns, built on first use, and a MINRES solve (scipy.sparse.linalg.minres) that runs on that product."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "sfbm_ref.c")
SO = os.path.join(HERE, "libsfbm_ref.so")
_lib = None

i64p, i32p, f64p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(SRC):
        cc = os.environ.get("CC", "gcc")
        base = [cc, "-O3", "-std=c99", "-fPIC", "-shared", SRC, "-o", SO + ".tmp"]
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
        lib.sfbm_prodvec.restype = None
        lib.sfbm_prodvec.argtypes = [i64p, i32p, f64p, C.c_int64, f64p, f64p, C.c_int]
        lib.sfbm_colsumsq.restype = None
        lib.sfbm_colsumsq.argtypes = [i64p, f64p, C.c_int64, f64p, C.c_int]
        _lib = lib
    return _lib


class Matrix:
    """full columns p (int64), i (int32), x (float64) of a symmetric matrix"""

    def __init__(self, p, i, x, nthreads=16):
        self.p, self.i, self.x = (np.ascontiguousarray(a, dtype=t) for a, t in ((p, np.int64), (i, np.int32), (x, np.float64)))
        self.m = self.p.size - 1
        self.nthreads = nthreads

    def prodvec(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        y = np.empty(self.m)
        load().sfbm_prodvec(self.p.ctypes.data_as(i64p), self.i.ctypes.data_as(i32p), self.x.ctypes.data_as(f64p), self.m,
                            v.ctypes.data_as(f64p), y.ctypes.data_as(f64p), self.nthreads)
        return y

    def colsumsq(self):
        y = np.empty(self.m)
        load().sfbm_colsumsq(self.p.ctypes.data_as(i64p), self.x.ctypes.data_as(f64p), self.m, y.ctypes.data_as(f64p),
                             self.nthreads)
        return y

    def solve_sym(self, b, add_to_diag, tol=1e-10, maxiter=None):
        """(A + diag(add_to_diag)) x = b by scipy's MINRES over prodvec; returns x, products made, true relative residual"""
        from scipy.sparse.linalg import LinearOperator, minres
        d = np.broadcast_to(np.asarray(add_to_diag, dtype=np.float64), (self.m,))
        count = [0]

        def mv(v):
            count[0] += 1
            return self.prodvec(v) + d * np.ravel(v)

        op = LinearOperator((self.m, self.m), matvec=mv, dtype=np.float64)
        try:
            x, _ = minres(op, b, rtol=tol, maxiter=maxiter or 10 * self.m)
        except TypeError:          # older scipy: the argument is called tol
            x, _ = minres(op, b, tol=tol, maxiter=maxiter or 10 * self.m)
        products = count[0]
        return x, products, float(np.linalg.norm(b - mv(x)) / np.linalg.norm(b))
