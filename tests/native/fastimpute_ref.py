"""The CPU statement of snp_fastImpute (fastimpute_ref.cpp, over bigsnpr_amd/csrc/fastimpute_step.hpp) for the tests and
tools/probe_fastimpute.py: built on first use with g++ -O2 -ffp-contract=off (OpenMP over targets when the compiler has
it).  It takes an FBM's bytes (n x m, 0 / 1 / 2 = call, 3 = missing) and the predictor lists as offsets and indices, and
returns the bytes with 4 + call at the imputed positions, and the 2 x m infos."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "fastimpute_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("fastimpute_step.hpp", "impute_step.hpp", "gibbs_step.hpp")]
SO = os.path.join(HERE, "libfastimpute_ref.so")
NODES = 31
_lib = None

u8p, i32p, i64p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


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
        lib.fast_impute_ref.restype = C.c_int64
        lib.fast_impute_ref.argtypes = [u8p, C.c_int64, C.c_int64, i64p, i32p, C.c_double, C.c_uint64, u8p, f64p, i32p, C.c_int]
        _lib = lib
    return _lib


def lists(preds):
    """a list of m index sequences -> (pred_off int64 [m + 1], pred_idx int32)"""
    off = np.zeros(len(preds) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in preds])
    idx = np.concatenate([np.asarray(p, dtype=np.int32).ravel() for p in preds] + [np.zeros(0, dtype=np.int32)])
    return off, np.ascontiguousarray(idx, dtype=np.int32)


def fast_impute(bytes_nm, pred_off, pred_idx, p_train, seed, nthreads=1, trace=False):
    """(FBM bytes afterwards, infos 2 x m, number of variants without an observed call[, first-round trees m x 31 x 3])"""
    a = np.asfortranarray(np.asarray(bytes_nm, dtype=np.uint8))
    if a.ndim == 1:
        a = np.asfortranarray(a[:, None])
    n, m = a.shape
    off = np.ascontiguousarray(pred_off, dtype=np.int64)
    idx = np.ascontiguousarray(pred_idx, dtype=np.int32)
    assert off.shape == (m + 1,) and off[0] == 0 and off[-1] == idx.size
    out = np.empty((n, m), dtype=np.uint8, order="F")
    infos = np.empty((2, m), dtype=np.float64)
    tr = np.full((m, NODES, 3), -2, dtype=np.int32) if trace else None
    n_all = load().fast_impute_ref(a.ctypes.data_as(u8p), n, m, off.ctypes.data_as(i64p), idx.ctypes.data_as(i32p),
                                   float(p_train), int(seed) & (2 ** 64 - 1), out.ctypes.data_as(u8p),
                                   infos.ctypes.data_as(f64p), None if tr is None else tr.ctypes.data_as(i32p), int(nthreads))
    return (out, infos, int(n_all), tr) if trace else (out, infos, int(n_all))
