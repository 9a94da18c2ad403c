"""The CPU statement of AUC / AUCBoot (auc_ref.cpp, over bigsnpr_amd/csrc/auc_step.hpp) for the tests and
tools/probe_auc.py: built on first use with g++ -O2 -ffp-contract=off -fopenmp.  Beside it, the definitions the tests
hold everything against, in numpy integers and independent of the header: auc_definition, philox_rows."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "auc_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "auc_step.hpp"), os.path.join(CSRC, "gibbs_step.hpp")]
SO = os.path.join(HERE, "libauc_ref.so")
TAG = 0x41554342
_lib = None

f64p, i32p, u8p, u64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
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
        lib.auc_twin.restype = i64
        lib.auc_twin.argtypes = [f64p, i64, i64, i64, u8p, u64p, f64p]
        lib.auc_draws.restype = None
        lib.auc_draws.argtypes = [i64, i64, C.c_uint64, i32p]
        lib.auc_boot_twin.restype = i64
        lib.auc_boot_twin.argtypes = [f64p, i64, i64, i64, u8p, i64, C.c_uint64, f64p]
        lib.auc_order_key.restype = C.c_uint64
        lib.auc_order_key.argtypes = [C.c_double]
        lib.auc_draw_tag.restype = C.c_uint32
        _lib = lib
    return _lib


def _xy(pred, target):
    x = np.asfortranarray(np.asarray(pred, dtype=np.float64))
    if x.ndim == 1:
        x = np.asfortranarray(x[:, None])
    y = np.ascontiguousarray(target, dtype=np.uint8)
    assert y.size == x.shape[0]
    return x, y


def auc(pred, target):
    """dict(auc: K doubles, counts: K x 3 uint64 (twoU, n1, n0)); a NaN raises ValueError naming the first such column"""
    x, y = _xy(pred, target)
    n, K = x.shape
    counts = np.zeros((K, 3), dtype=np.uint64)
    out = np.zeros(K)
    bad = load().auc_twin(x.ctypes.data_as(f64p), max(n, 1), n, K, y.ctypes.data_as(u8p), counts.ctypes.data_as(u64p),
                          out.ctypes.data_as(f64p))
    if bad >= 0:
        raise ValueError("NaN in column %d" % bad)
    return dict(auc=out, counts=counts)


def draws(n, b, seed):
    rows = np.zeros(n, dtype=np.int32)
    load().auc_draws(n, b, C.c_uint64(seed), rows.ctypes.data_as(i32p))
    return rows


def boot(pred, target, nboot, seed):
    """the replicates, nboot x K"""
    x, y = _xy(pred, target)
    n, K = x.shape
    rep = np.zeros((nboot, K), order="F")
    bad = load().auc_boot_twin(x.ctypes.data_as(f64p), max(n, 1), n, K, y.ctypes.data_as(u8p), nboot, C.c_uint64(seed),
                               rep.ctypes.data_as(f64p))
    if bad >= 0:
        raise ValueError("NaN in column %d" % bad)
    return rep


# ---- the definitions, independent of the header ----------------------------------------------------------------------------
def two_u_definition(x, y):
    """(twoU, n1, n0) over all (case, control) pairs in Python integers.  O(n1 n0) in blocks of cases."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y)
    cases, controls = x[y == 1], x[y == 0]
    two_u = 0
    for i0 in range(0, cases.size, 2048):
        c = cases[i0:i0 + 2048, None]
        two_u += 2 * int((c > controls[None, :]).sum()) + int((c == controls[None, :]).sum())
    return two_u, int(cases.size), int(controls.size)


def auc_definition(x, y):
    """the definition as one double: twoU / (2 n1 n0), NaN without a case or without a control"""
    two_u, n1, n0 = two_u_definition(x, y)
    if n1 == 0 or n0 == 0:
        return np.nan
    return float(np.float64(two_u) / (np.float64(2.0) * (np.float64(n1) * np.float64(n0))))


def philox_rows(philox4x32_10, n, b, seed):
    """the rows replicate b draws, restated in numpy with a philox4x32_10(c, k) on arrays (tests/test_impute_cpu.py's)"""
    t = np.arange(n, dtype=np.uint64)
    q = t >> np.uint64(2)
    z = np.zeros(n, dtype=np.uint64)
    o = philox4x32_10([q, z + np.uint64(b), z + np.uint64(TAG), z], (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    words = np.stack([np.asarray(w, dtype=np.uint64) for w in o])          # 4 x n
    word = words[(t & np.uint64(3)).astype(np.int64), np.arange(n)]
    return ((word * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
