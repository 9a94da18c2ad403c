"""The host build of k_cprod's one-dimensional grid (bigsnpr_amd/csrc/prod_plan.hpp through cprod_grid_ref.cpp) for
tests/test_cprod_grid_cpu.py and tests/test_gpu_cprod_whole.py: built on first use with g++ -O2."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "cprod_grid_ref.cpp")
HDRS = [os.path.join(ROOT, "bigsnpr_amd", "csrc", f) for f in ("prod_plan.hpp", "byte_plan.hpp")]
SO = os.path.join(HERE, "libcprod_grid_ref.so")
_lib = None

FIELDS = ("m", "per_wg", "nchunks", "pitch", "NB", "nplane", "ncu", "resident", "one_split", "slabs")
OUT = ("blocks", "blocks_whole", "slabs", "cps", "nchunks", "m_rem", "workgroups", "partial_words")


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        cxx = os.environ.get("CXX", "g++")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDRS[0]), SRC,
                               "-o", SO + ".tmp"])
        os.replace(SO + ".tmp", SO)
    return SO


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        lib.cg_plan.restype = None
        lib.cg_plan.argtypes = [C.c_void_p, C.c_void_p]
        lib.cg_slab.restype = None
        lib.cg_slab.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.cg_check.restype = C.c_int
        lib.cg_check.argtypes = [C.c_void_p]
        _lib = lib
    return _lib


def facts(n, m, NB, nplane=2, ncu=256, resident=None, one_split=0, slabs=0):
    """the facts of a launch over m contiguous variants of an image of n samples: a workgroup has 256 variants with one column
    block and 512 with two or three; `resident` defaults to what the kernels' register budgets allow (2 and 1)"""
    nchunks = (n + 1023) // 1024 * 2        # (a variant's row is padded to 1 024 samples)
    return dict(m=m, per_wg=256 if NB == 1 else 512, nchunks=nchunks, pitch=nchunks * 128, NB=NB, nplane=nplane, ncu=ncu,
                resident=resident if resident is not None else (2 if NB == 1 else 1), one_split=one_split, slabs=slabs)


def _facts(kw):
    assert set(kw) == set(FIELDS), sorted(set(kw) ^ set(FIELDS))
    return np.array([kw[k] for k in FIELDS], dtype=np.int64)


def plan(**kw):
    """plan_cprod's answer as a dict (OUT)"""
    f, out = _facts(kw), np.zeros(len(OUT), dtype=np.int64)
    load().cg_plan(f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return dict(zip(OUT, (int(v) for v in out)))


def slab(wg, **kw):
    """(block, slab, first chunk, end chunk) of workgroup wg in the plan's grid"""
    f, out = _facts(kw), np.zeros(4, dtype=np.int64)
    load().cg_slab(f.ctypes.data_as(C.c_void_p), int(wg), out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def check(**kw):
    """0 when the grid of the plan covers every (block, chunk) once and the partial region without overlap or gap
    (cprod_grid_ref.cpp: cg_check), otherwise the number of the rule broken"""
    f = _facts(kw)
    return int(load().cg_check(f.ctypes.data_as(C.c_void_p)))
