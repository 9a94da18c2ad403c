"""Seeded inputs for snp_ldsplit's kernels (bigsnpr_amd/csrc/ldsplit.hip).  Banded symmetric matrices with unit diagonal
whose off-diagonals are drawn from {0, +-0.25, +-0.5}: every r^2 is 0, 1/16 or 1/4, every sum of them an exact dyadic (in
the float of E as well: all sums here stay far below 2^20), so equal costs are equal bit for bit and ties are frequent.
tests/test_ldsplit_cpu.py proves on the CPU statement, with its counters, that each named input contains what it is for;
tests/test_gpu_ldsplit.py runs the device on them."""
import os
import re

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LDSPLIT = os.path.join(ROOT, "bigsnpr_amd", "csrc", "ldsplit.hip")

CONSTANTS = ("kThreads", "kRowTile", "kSplit")


def kernel_constants():
    """the `constexpr` integers of ldsplit.hip that decide its tiles"""
    with open(LDSPLIT) as f:
        src = f.read()
    out = {}
    for name in CONSTANTS:
        found = re.findall(r"^\s*constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src, flags=re.M)
        assert len(found) == 1, "%s: %d constexpr lines in %s" % (name, len(found), LDSPLIT)
        out[name] = int(found[0])
    return out


def banded(m, band, seed, p_zero=0.4, p_half=0.1):
    """symmetric, unit diagonal, |i - j| <= band; an off-diagonal is 0 with probability p_zero (not stored), +-0.5 with
    p_half, else +-0.25"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for d in range(1, band + 1):
        n = m - d
        if n <= 0:
            break
        u = rng.random(n)
        mag = np.where(u < p_zero, 0.0, np.where(u < p_zero + p_half, 0.5, 0.25))
        v = mag * rng.choice([-1.0, 1.0], n)
        keep = v != 0
        rows.append(np.arange(n)[keep])
        cols.append(np.arange(n)[keep] + d)
        vals.append(v[keep])
    up = sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m, m))
    A = sparse.csc_matrix(up + up.T + sparse.identity(m))
    A.sort_indices()
    return A


def isolate(A, j):
    """column and row j keep their diagonal only"""
    L = sparse.lil_matrix(A)
    L[j, :] = 0
    L[:, j] = 0
    L[j, j] = 1.0
    B = sparse.csc_matrix(L)
    B.eliminate_zeros()
    B.sort_indices()
    return B


def named(name):
    """(matrix, keyword arguments of one dynamic program) of a named input.  The shapes follow the tiles of ldsplit.hip: m
    one above, one below and at a multiple of the row tile, W = max_size - min_size + 1 more than four passes of the split
    of a row's t range."""
    inf = float("inf")
    k = kernel_constants()
    tile, wide = k["kRowTile"], 4 * k["kSplit"] + 3
    if name == "ties":          # candidates decided by cost2 at equal cost1, and full ties
        return banded(3 * tile + 1, 4, 11), dict(thr_r2=0.0, min_size=2, max_size=2 + wide, max_K=30, max_r2=1.0, max_cost=inf)
    if name == "max_r2":        # pairs that no split may separate: +-0.5 about once per 30 columns
        return banded(3 * tile - 1, 3, 12, p_zero=0.5, p_half=1 / 90), dict(thr_r2=0.0, min_size=2, max_size=2 + wide, max_K=25,
                                                                             max_r2=0.1, max_cost=inf)
    if name == "early_stop":    # the levels end strictly before max_K
        return banded(150, 5, 13, p_zero=0.8), dict(thr_r2=0.0, min_size=3, max_size=12, max_K=60, max_r2=1.0, max_cost=4.0)
    if name == "window":        # 20 variants per unit of position: the window cuts E and level 0
        m = 3 * tile
        return banded(m, 4, 14), dict(thr_r2=0.0, min_size=2, max_size=2 + wide, max_K=30, max_r2=1.0, max_cost=inf,
                                      pos_scaled=np.arange(m) / 20.0)
    if name == "diagonal_only":     # column 57 stores its diagonal only; min_size = 1
        return isolate(banded(130, 4, 15), 57), dict(thr_r2=0.0, min_size=1, max_size=25, max_K=20, max_r2=1.0, max_cost=inf)
    if name == "thr_r2":        # 1/16 is ignored, 1/4 counts
        return banded(200, 4, 16, p_half=0.3), dict(thr_r2=0.1, min_size=2, max_size=30, max_K=30, max_r2=1.0, max_cost=inf)
    if name == "W_is_1":        # blocks of six; more levels than are feasible
        m = 3 * tile
        return banded(m, 4, 11), dict(thr_r2=0.0, min_size=6, max_size=6, max_K=m // 6 + 8, max_r2=1.0, max_cost=inf)
    if name == "max_size_is_m":
        return banded(tile + 1, 4, 11), dict(thr_r2=0.0, min_size=1, max_size=tile + 1, max_K=12, max_r2=1.0, max_cost=inf)
    if name == "level_0_only":
        return banded(tile + 1, 4, 11), dict(thr_r2=0.0, min_size=1, max_size=tile + 1, max_K=1, max_r2=1.0, max_cost=inf)
    if name == "moderate":      # 47 row tiles, W = 301
        return banded(47 * tile - 7, 6, 21), dict(thr_r2=0.0, min_size=50, max_size=350, max_K=60, max_r2=1.0, max_cost=inf)
    raise KeyError(name)


NAMES = ("ties", "max_r2", "early_stop", "window", "diagonal_only", "thr_r2", "W_is_1", "max_size_is_m", "level_0_only",
         "moderate")


def outside_cost(A, all_last, thr_r2):
    """the sum of r^2 >= thr_r2 over the lower-triangle entries whose ends lie in different blocks (all_last: the 0-based
    last index of each block), and the largest such r^2 — straight from the matrix, in numpy"""
    T = sparse.coo_matrix(sparse.tril(A, k=-1))
    block = np.searchsorted(np.asarray(all_last), np.arange(A.shape[0]), side="left")
    r2 = T.data * T.data
    out = (block[T.row] != block[T.col]) & (r2 >= thr_r2)
    return float(np.sum(r2[out])), float(np.max(r2[out])) if out.any() else 0.0
