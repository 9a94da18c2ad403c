"""snp_ldsplit on the device — host mirror of R/split-LD.R over the resident sparse LD matrix (SFBM).

bsn_sfbm_ldsplit runs get_L, get_C, reconstruct_paths and get_perc for one max_size (csrc/ldsplit.hip); this module does
what snp_ldsplit does around them: the clamp of max_cost, the values of max_size in ascending order, and the rule that a
number of blocks is reported again only at a strictly lower cost.  Indices are 0-based."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f64p, i32p, ptr
from .lassosum2 import SFBM, as_SFBM

COLUMNS = ("max_size", "n_block", "cost", "cost2", "perc_kept", "all_last", "all_size")


def lower_sumsq(p, i, x, m2, upper):
    """sum of x^2 over the lower triangle with the diagonal (crossprod(tril(corr)@x)).  An upper triangle is the transposed
    lower one: all of its entries; full columns: the entries with row >= column."""
    x = np.asarray(x, dtype=np.float64)
    if upper:
        return float(np.dot(x, x))
    col = np.repeat(np.arange(m2, dtype=np.int64), np.diff(np.asarray(p, dtype=np.int64)))
    xl = x[np.asarray(i) >= col]
    return float(np.dot(xl, xl))


def clamp_max_cost(max_cost, m, sumsq_lower):
    """R/split-LD.R: max_cost defaults to ncol(corr) / 200 and is at most twice the lower triangle's sum of squares (so
    that max_cost = Inf is allowed)"""
    max_cost = m / 200 if max_cost is None else float(max_cost)
    return min(max_cost, 2 * sumsq_lower)


def ldsplit_rows(run_one, max_sizes, max_K):
    """The loop of snp_ldsplit over sort(max_size).  run_one(max_size) returns the outputs of one dynamic program: cost,
    cost2, perc_kept, ok [max_K] and all_last [max_K x max_K] (best_ind along the path).  K blocks are reported when they
    were reconstructed and cost strictly less than what a smaller max_size already reported for K.  Returns the dict of
    columns, or None when no row qualifies."""
    prev = np.full(max_K, np.inf)
    out = {c: [] for c in COLUMNS}
    for one in sorted(int(v) for v in np.atleast_1d(max_sizes)):
        r = run_one(one)
        for kk in range(max_K):
            cost = float(r["cost"][kk])
            if not r["ok"][kk] or not cost < prev[kk]:
                continue
            prev[kk] = cost
            nxt = np.asarray(r["all_last"][kk, :kk + 1], dtype=np.int64)   # first row of the block behind each block
            out["max_size"].append(one)
            out["n_block"].append(kk + 1)
            out["cost"].append(cost)
            out["cost2"].append(float(r["cost2"][kk]))
            out["perc_kept"].append(float(r["perc_kept"][kk]))
            out["all_last"].append(nxt - 1)
            out["all_size"].append(np.diff(np.concatenate([[0], nxt])))
    if not out["n_block"]:
        return None
    for c in ("max_size", "n_block"):
        out[c] = np.array(out[c], dtype=np.int64)
    for c in ("cost", "cost2", "perc_kept"):
        out[c] = np.array(out[c], dtype=np.float64)
    return out


def ldsplit_one(sf, thr_r2, min_size, max_size, max_K, max_r2, max_cost, pos_scaled=None, tables=True):
    """One call of bsn_sfbm_ldsplit on the resident matrix `sf` with max_cost as given (no clamp): a dict with C and
    best_ind [m x max_K] (when `tables`), cost, cost2, perc_kept, ok [max_K], all_last [max_K x max_K], levels_run and
    seconds (E, levels, epilogue)."""
    m, K = sf.ncol, int(max_K)
    pos = None if pos_scaled is None else np.ascontiguousarray(np.ravel(pos_scaled), dtype=np.float64)
    if pos is not None and pos.size != m:
        raise ValueError("'pos_scaled' should have one element per column of 'corr'.")
    Kn = max(K, 0)
    res = {"cost": np.empty(Kn), "cost2": np.empty(Kn), "perc_kept": np.empty(Kn), "ok": np.zeros(Kn, dtype=np.int32),
           "all_last": np.empty((Kn, Kn), dtype=np.int32), "seconds": np.zeros(3)}
    if tables:
        res["C"] = np.empty((m, Kn), order="F")
        res["best_ind"] = np.empty((m, Kn), dtype=np.int32, order="F")
    levels = C.c_int32(0)
    check(_lib.load().bsn_sfbm_ldsplit(sf.handle, float(thr_r2), float(max_r2), int(min_size), int(max_size), K,
                                       float(max_cost), ptr(pos, f64p), ptr(res.get("C"), f64p),
                                       ptr(res.get("best_ind"), i32p), ptr(res["cost"], f64p), ptr(res["cost2"], f64p),
                                       ptr(res["perc_kept"], f64p), ptr(res["ok"], i32p), ptr(res["all_last"], i32p),
                                       C.byref(levels), ptr(res["seconds"], f64p)))
    res["levels_run"] = levels.value
    return res


def snp_ldsplit(corr, thr_r2, min_size, max_size, max_K=500, max_r2=0.3, max_cost=None, pos_scaled=None):
    """R/split-LD.R snp_ldsplit.  corr: an SFBM or anything as_SFBM takes (converted for this call only); max_size: one
    value or several.  Returns None when no split satisfies the conditions, else a dict of the columns max_size, n_block,
    cost, cost2, perc_kept (arrays) and all_last, all_size (one array per row; all_last is the 0-based last index of each
    block)."""
    own = not isinstance(corr, SFBM)
    sf = as_SFBM(corr)
    try:
        mc = clamp_max_cost(max_cost, sf.ncol, sf.sumsq_lower)
        return ldsplit_rows(lambda one: ldsplit_one(sf, thr_r2, min_size, one, max_K, max_r2, mc, pos_scaled, tables=False),
                            max_size, int(max_K))
    finally:
        if own:
            sf.close()
