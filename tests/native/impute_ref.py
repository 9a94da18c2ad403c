"""The CPU statement of snp_fastImputeSimple (impute_ref.cpp, over bigsnpr_amd/csrc/impute_step.hpp) for the tests and
tools/probe_impute.py: built on first use with g++ -O2 -ffp-contract=off (OpenMP over variants when the compiler has it).
It takes and returns an FBM's bytes: n x m, 0 / 1 / 2 = call, 3 = missing; 4 + call / 7 + r at an imputed position."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "impute_ref.cpp")
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, "impute_step.hpp"), os.path.join(CSRC, "gibbs_step.hpp")]
SO = os.path.join(HERE, "libimpute_ref.so")
METHODS = {"zero": 0, "mode": 1, "mean0": 2, "mean2": 3, "random": 4}
_lib = None

u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


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
        lib.impute_simple_ref.restype = C.c_int64
        lib.impute_simple_ref.argtypes = [u8p, C.c_int64, C.c_int64, C.c_int, C.c_uint64, u8p, i32p, C.c_int]
        lib.impute_rule_val.restype = C.c_int32
        lib.impute_rule_val.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64]
        lib.impute_rule_af.restype = C.c_double
        lib.impute_rule_af.argtypes = [C.c_int64, C.c_int64, C.c_int64]
        lib.impute_draw.restype = C.c_int
        lib.impute_draw.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_double]
        _lib = lib
    return _lib


def read_bed_bytes(bedfile, n, m):
    """the FBM bytes snp_readBed makes of a .bed file (n x m; 0 / 1 / 2 = call, 3 = missing), decoded in numpy:
    the 2-bit codes 00, 01, 10, 11 are 2, missing, 1, 0 (src/bed-acc.h:22-37)"""
    raw = np.fromfile(bedfile, dtype=np.uint8)
    assert raw[0] == 0x6C and raw[1] == 0x1B and raw[2] == 1
    nb = (n + 3) // 4
    pay = raw[3:].reshape(m, nb)
    codes = np.stack([(pay >> (2 * e)) & 3 for e in range(4)], axis=2).reshape(m, 4 * nb)[:, :n]
    return np.asfortranarray(np.array([2, 3, 1, 0], dtype=np.uint8)[codes].T)


SEED = 20240611   # `random` in the tests: chosen on the CPU (tests/test_impute_cpu.py says how)


def chi_square_column():
    """3000 samples, 1200 of them missing, allele frequency near 0.3 among the others"""
    rng = np.random.default_rng(7)
    col = rng.binomial(2, 0.3, 3000).astype(np.uint8)
    col[rng.choice(3000, 1200, replace=False)] = 3
    return col


def chi_square_pvalue(col, out):
    """goodness of fit of the imputed calls to ((1 - p)^2, 2 p (1 - p), p^2), p the observed allele frequency; two
    degrees of freedom, whose chi-square tail is exp(-x / 2)"""
    na = col == 3
    p = col[~na].mean() / 2
    prob = np.array([(1 - p) ** 2, 2 * p * (1 - p), p ** 2])
    obs = np.bincount(out[na].astype(np.int64) - 4, minlength=3)
    expd = prob * na.sum()
    return float(np.exp(-((obs - expd) ** 2 / expd).sum() / 2))


def impute(bytes_nm, method, seed=0, nthreads=1):
    """(FBM bytes after the reference's in-place rewrite, per-variant value of the rule, number of variants without a call)"""
    a = np.asfortranarray(np.asarray(bytes_nm, dtype=np.uint8))
    if a.ndim == 1:
        a = np.asfortranarray(a[:, None])
    n, m = a.shape
    out = np.empty((n, m), dtype=np.uint8, order="F")
    val = np.empty(m, dtype=np.int32)
    n_all = load().impute_simple_ref(a.ctypes.data_as(u8p), n, m, METHODS[method], int(seed) & (2 ** 64 - 1),
                                     out.ctypes.data_as(u8p), val.ctypes.data_as(i32p), int(nthreads))
    return out, val, int(n_all)


def rule_val(method, c1, c2, c):
    return int(load().impute_rule_val(METHODS[method], int(c1), int(c2), int(c)))


def rule_af(c1, c2, c):
    return float(load().impute_rule_af(int(c1), int(c2), int(c)))


def draw(seed, i, j, af):
    return int(load().impute_draw(int(seed) & (2 ** 64 - 1), int(i), int(j), float(af)))
