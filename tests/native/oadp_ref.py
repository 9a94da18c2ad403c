"""The CPU statement of the OADP projection (oadp_ref.cpp, over bigsnpr_amd/csrc/oadp_step.hpp) for the tests: built on
first use with g++ -O2."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "oadp_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "oadp_step.hpp")]
SO = os.path.join(HERE, "liboadp_ref.so")
_lib = None

f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        cxx = os.environ.get("CXX", "g++")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", CSRC, SRC, "-o", SO + ".tmp"])
        os.replace(SO + ".tmp", SO)
    return SO


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        lib.oadp_max_k.restype = C.c_int
        lib.oadp_sweep_cap.restype = C.c_int
        lib.oadp_check.restype = C.c_char_p
        lib.oadp_check.argtypes = [C.c_int64, f64p]
        lib.oadp_proj.restype = C.c_int
        lib.oadp_proj.argtypes = [f64p, f64p, f64p, C.c_int64, C.c_int64, f64p, i32p]
        _lib = lib
    return _lib


def max_k():
    return int(load().oadp_max_k())


def sweep_cap():
    return int(load().oadp_sweep_cap())


def proj(XV, X_norm, sval, return_sweeps=False):
    """pca_OADP_proj2(XV, X_norm, sval) by the header's statement; ValueError with the library's message when (K, sval)
    is refused"""
    XV = np.asfortranarray(np.asarray(XV, dtype=np.float64))
    X_norm = np.ascontiguousarray(np.ravel(X_norm), dtype=np.float64)
    sval = np.ascontiguousarray(np.ravel(sval), dtype=np.float64)
    n, K = XV.shape
    if sval.size != K or X_norm.size != n:
        raise ValueError("Incompatibility between dimensions.")
    why = load().oadp_check(K, sval.ctypes.data_as(f64p))
    if why is not None:
        raise ValueError(why.decode())
    out = np.empty((n, K), dtype=np.float64, order="F")
    sweeps = np.empty(n, dtype=np.int32)
    rc = load().oadp_proj(XV.ctypes.data_as(f64p), X_norm.ctypes.data_as(f64p), sval.ctypes.data_as(f64p), n, K,
                          out.ctypes.data_as(f64p), sweeps.ctypes.data_as(i32p))
    assert rc == 0
    return (out, sweeps) if return_sweeps else out
