"""The host build of k_prodT's one-dimensional grid (bigsnpr_amd/csrc/prod_plan.hpp through prodt_grid_ref.cpp) for
tests/test_prodt_grid_cpu.py: built on first use with g++ -O2."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "prodt_grid_ref.cpp")
HDRS = [os.path.join(ROOT, "bigsnpr_amd", "csrc", f) for f in ("prod_plan.hpp", "byte_plan.hpp")]
SO = os.path.join(HERE, "libprodt_grid_ref.so")
_lib = None

FIELDS = ("bits", "n", "m", "pitch", "col0", "cols_contig", "have_smaj", "mode", "raw_na", "has_q", "no_sparse", "nvec", "S", "ncu",
          "segmented", "ky", "ky_t", "ky_whole")
OUT = ("refuse", "smaj", "vmax", "m_pad", "wgx", "ky", "smaj_cps", "mc", "sparse_ok", "wgx_whole", "ky_whole", "cps_whole", "workgroups")


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
        lib.pg_plan.restype = None
        lib.pg_plan.argtypes = [C.c_void_p, C.c_void_p]
        lib.pg_slab.restype = None
        lib.pg_slab.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.pg_check.restype = C.c_int
        lib.pg_check.argtypes = [C.c_void_p]
        _lib = lib
    return _lib


def _facts(kw):
    assert set(kw) <= set(FIELDS), sorted(set(kw) - set(FIELDS))
    return np.array([kw.get(k, 0) for k in FIELDS], dtype=np.int64)


def plan(**kw):
    """plan_prod's answer as a dict (OUT)"""
    f, out = _facts(kw), np.zeros(len(OUT), dtype=np.int64)
    load().pg_plan(f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return dict(zip(OUT, (int(v) for v in out)))


def slab(wg, **kw):
    """(sample block, slab, first chunk, end chunk) of workgroup wg in the plan's grid"""
    f, out = _facts(kw), np.zeros(4, dtype=np.int64)
    load().pg_slab(f.ctypes.data_as(C.c_void_p), int(wg), out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def check(**kw):
    """0 when the grid of the plan covers every (sample block, chunk) once within the rules (prodt_grid_ref.cpp: pg_check),
    -1 when the plan is not k_prodT's, otherwise the number of the rule broken"""
    f = _facts(kw)
    return int(load().pg_check(f.ctypes.data_as(C.c_void_p)))
