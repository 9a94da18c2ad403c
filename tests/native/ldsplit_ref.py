"""The CPU statement of snp_ldsplit (ldsplit_ref.cpp, over bigsnpr_amd/csrc/ldsplit_step.hpp) for the tests and
tools/probe_ldsplit.py: built on first use with g++ -O2 -ffp-contract=off, plus a short pure-Python transliteration of the
rules (a dictionary for L, lists for E) that the C statement is checked against on tiny cases, and snp_ldsplit itself over
the statement: the host mirror's own clamp and loop over max_size with `split` in the place of the device call."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "ldsplit_ref.cpp")
HDR = os.path.join(ROOT, "bigsnpr_amd", "csrc", "ldsplit_step.hpp")
SO = os.path.join(HERE, "libldsplit_ref.so")
_lib = None

i64p, i32p, f64p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)

COUNTERS = ("by_cost2", "full_tie", "best_with_inf", "E_window", "level0_window", "E_max_cost", "finite_levels",
            "diagonal_only")


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        cxx = os.environ.get("CXX", "g++")
        subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I",
                               os.path.dirname(HDR), SRC, "-o", SO + ".tmp"])
        os.replace(SO + ".tmp", SO)
    return SO


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        lib.lds_split.restype = C.c_int64
        lib.lds_split.argtypes = [i64p, i32p, f64p, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_double, f64p, f64p, i32p, f64p, f64p, f64p, i32p, i32p, i32p, i64p]
        lib.lds_gather.restype = C.c_int32
        lib.lds_gather.argtypes = [i64p, i32p, f64p, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_double, f64p, C.c_int32, f64p, i32p]
        _lib = lib
    return _lib


def csc(A):
    """(p, i, x) of a scipy matrix with ascending rows: the statement reads the diagonal and what is below it"""
    from scipy import sparse
    A = sparse.csc_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)


def split(p, i, x, m, thr_r2, min_size, max_size, max_K, max_r2, max_cost, pos_scaled=None, counters=True):
    """one dynamic program: the outputs of bsn_sfbm_ldsplit under the same names, plus `counters` (COUNTERS; they cost a
    second pass over every level's candidates, which a timing run leaves out)"""
    L = load()
    p, i, x = (np.ascontiguousarray(a, dtype=t) for a, t in ((p, np.int64), (i, np.int32), (x, np.float64)))
    pos = None if pos_scaled is None else np.ascontiguousarray(pos_scaled, dtype=np.float64)
    K = int(max_K)
    res = {"C": np.empty((m, K), order="F"), "best_ind": np.empty((m, K), dtype=np.int32, order="F"), "cost": np.empty(K),
           "cost2": np.empty(K), "perc_kept": np.empty(K), "ok": np.zeros(K, dtype=np.int32),
           "all_last": np.empty((K, K), dtype=np.int32)}
    levels = C.c_int32(0)
    cnt = np.zeros(len(COUNTERS), dtype=np.int64) if counters else None
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    rc = L.lds_split(ptr(p, i64p), ptr(i, i32p), ptr(x, f64p), int(m), float(thr_r2), float(max_r2), int(min_size),
                     int(max_size), K, float(max_cost), ptr(pos, f64p), ptr(res["C"], f64p), ptr(res["best_ind"], i32p),
                     ptr(res["cost"], f64p), ptr(res["cost2"], f64p), ptr(res["perc_kept"], f64p), ptr(res["ok"], i32p),
                     ptr(res["all_last"], i32p), C.byref(levels), ptr(cnt, i64p))
    if rc:
        raise ValueError("column %d has no non-zero diagonal" % (rc - 1))
    res["levels_run"] = levels.value
    if counters:
        res["counters"] = dict(zip(COUNTERS, (int(v) for v in cnt)))
    return res


def gather(p, i, x, m, thr_r2, min_size, max_size, max_K, max_r2, max_cost, pos_scaled=None, split=1):
    """the levels by the kernels' per-row gather in the order of ldsplit_step.hpp, `split` partial minima per row, on the
    host: (C, best_ind, levels_run)"""
    L = load()
    p, i, x = (np.ascontiguousarray(a, dtype=t) for a, t in ((p, np.int64), (i, np.int32), (x, np.float64)))
    pos = None if pos_scaled is None else np.ascontiguousarray(pos_scaled, dtype=np.float64)
    Cm = np.empty((m, int(max_K)), order="F")
    best = np.empty((m, int(max_K)), dtype=np.int32, order="F")
    levels = L.lds_gather(p.ctypes.data_as(i64p), i.ctypes.data_as(i32p), x.ctypes.data_as(f64p), int(m), float(thr_r2),
                          float(max_r2), int(min_size), int(max_size), int(max_K), float(max_cost),
                          None if pos is None else pos.ctypes.data_as(f64p), int(split), Cm.ctypes.data_as(f64p),
                          best.ctypes.data_as(i32p))
    return Cm, best, levels


def snp_ldsplit(A, thr_r2, min_size, max_size, max_K=500, max_r2=0.3, max_cost=None, pos_scaled=None):
    """bigsnpr_amd.snp_ldsplit with the statement behind it (A: a scipy matrix holding at least the lower triangle)"""
    from scipy import sparse
    from bigsnpr_amd.ldsplit import clamp_max_cost, ldsplit_rows, lower_sumsq
    p, i, x = csc(sparse.tril(sparse.csc_matrix(A)))
    m = A.shape[1]
    if not (min_size >= 1 and np.all(np.atleast_1d(max_size) <= m)):
        raise ValueError("min_size >= 1 && all(max_size <= m) is not TRUE")
    mc = clamp_max_cost(max_cost, m, lower_sumsq(p, i, x, m, False))
    return ldsplit_rows(lambda one: split(p, i, x, m, thr_r2, min_size, one, max_K, max_r2, mc, pos_scaled), max_size, int(max_K))


def py_split(p, i, x, m, thr_r2, min_size, max_size, max_K, max_r2, max_cost, pos_scaled=None):
    """rules 1 - 5 in Python floats (IEEE doubles, every operation rounded): (C [m x max_K], best_ind [m x max_K], levels)"""
    inf = float("inf")
    pos = [0.0] * m if pos_scaled is None else [float(v) for v in pos_scaled]
    L = {}
    for c in range(m):
        l = 0.0
        for e in range(int(p[c + 1]) - 1, int(p[c]) - 1, -1):
            if int(i[e]) <= c:
                break
            r2 = float(x[e]) * float(x[e])
            if r2 >= thr_r2:
                l = inf if r2 > max_r2 else l + r2
            lo = int(i[e - 1]) if int(i[e - 1]) > c else c      # l holds down to the next stored row (or the diagonal)
            for row in range(int(i[e]), lo, -1):
                if l > 0:
                    L[(c, row)] = l
    E = []
    for col in range(m):
        e, count, kept = 0.0, 0, []
        for row in range(col, -1, -1):
            if pos[row] < pos[col] - 1:
                break
            e = e + L.get((row, col + 1), 0.0)
            if e > max_cost:
                break
            count += 1
            if count >= min_size:
                kept.append(float(np.float32(e)))
                if count == max_size:
                    break
        E.append(kept)
    C1 = np.full((m + 1, max_K), inf)
    C2 = np.full((m + 1, max_K), inf)
    best = np.full((m, max_K), -1, dtype=np.int32)
    for size in range(min_size, max_size + 1):
        row = m - size
        if pos[row] < pos[m - 1] - 1:
            break
        best[row, 0], C1[row, 0], C2[row, 0] = m, 0.0, float(size) ** 2
    levels = max_K
    for k in range(1, max_K):
        for col in range(m - 1, -1, -1):
            for t, e in enumerate(E[col]):
                row = col - min_size + 1 - t
                cost1 = e + C1[col + 1, k - 1]
                cost2 = float(col - row + 1) ** 2 + C2[col + 1, k - 1]
                if cost1 < C1[row, k]:
                    best[row, k], C1[row, k], C2[row, k] = col + 1, cost1, cost2
                elif cost1 == C1[row, k] and cost2 < C2[row, k]:
                    best[row, k], C2[row, k] = col + 1, cost2
        if C1[0, k] > max_cost and C1[0, k] > C1[0, k - 1]:
            levels = k + 1
            break
    return C1[:m], best, levels
