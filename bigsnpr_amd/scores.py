"""big_prodMat / AUC / AUCBoot / pcor / snp_grid_AUC — from a grid of effect sizes to the chosen model and its interval,
host mirror of what the reference's tests and vignettes do with bigstatsr after every method that returns a grid
(tests/testthat/test-8-LDpred2.R:57, vignettes/SCT.Rmd:160-220) over bsn_bed_prodmat / bsn_auc / bsn_auc_boot /
bsn_pcor_moments (csrc/auc.hip, the rule in csrc/auc_step.hpp).

PARITY STATUS of this module: bigstatsr is external to the reference tree and no R is at hand.  `AUC` is pinned by its
definition (exact integers); `AUCBoot` does NOT emulate R's sample(): its resample rule is stated in auc_step.hpp, so its
replicates are this library's, its statistics those of any bootstrap; `pcor` follows the stated rule
r = cor(resid(x ~ 1 + z), resid(y ~ 1 + z)) with the Fisher interval.  Indices are 0-based."""
import ctypes as C
import os
from statistics import NormalDist

import numpy as np

from . import _lib
from ._lib import DeviceArray, check, f64p, i32p, i64p, ptr, u8p, vp
from .bed import ERROR_DIM

MAX_ROWS = 2 ** 31 - 1
MAX_COVAR = 31


def auc_last_ms():
    """device milliseconds of the last call of this module in this process: [key pass, sort, group + evaluation kernels,
    bootstrap kernel, pcor passes]"""
    ms = np.zeros(5)
    check(_lib.load().bsn_auc_last_ms(ptr(ms, f64p)))
    return ms


# ---- big_prodMat ---------------------------------------------------------------------------------------------------------
def big_prodMat(G, A, ind_row=None, ind_col=None, center=None, scale=None, on_device=False):
    """bigstatsr::big_prodMat on a `bed`, an `FBM_code256` or a dosage image: ((G[ind_row, ind_col] - center) / scale) A,
    n x K, through the product pass of prod_and_rowSumsSq.  A column of `A` that holds a NaN (a grid point that diverged)
    comes back as a column of NaN.  on_device=True: a DeviceArray that AUC / AUCBoot / pcor take without a download."""
    from .ld import _ind
    im, ir, ic = _ind(G, ind_row, ind_col)
    A = np.asarray(A, dtype=np.float64)
    if A.ndim == 1:
        A = A[:, None]
    if A.ndim != 2:
        raise ValueError("'A.col' should be a vector or a matrix.")
    A = np.asfortranarray(A)
    if A.shape[0] != ic.size:
        raise ValueError(ERROR_DIM)
    if A.shape[1] < 1:
        raise ValueError("'A.col' must have at least one column.")
    if (center is None) != (scale is None):
        center = np.zeros(ic.size) if center is None else center
        scale = np.ones(ic.size) if scale is None else scale
    if center is not None:
        center = np.ascontiguousarray(np.ravel(center), dtype=np.float64)
        scale = np.ascontiguousarray(np.ravel(scale), dtype=np.float64)
        if center.size != ic.size or scale.size != ic.size:
            raise ValueError(ERROR_DIM)
    n, K = ir.size, A.shape[1]
    lib = _lib.load()
    if on_device:
        out = DeviceArray(n, K)
        check(lib.bsn_bed_prodmat(im.handle, ptr(ir, i64p), n, ptr(ic, i64p), ic.size, ptr(center, f64p), ptr(scale, f64p),
                                  ptr(A, f64p), K, None, out.ptr))
        return out
    XV = np.empty((n, K), order="F")
    check(lib.bsn_bed_prodmat(im.handle, ptr(ir, i64p), n, ptr(ic, i64p), ic.size, ptr(center, f64p), ptr(scale, f64p),
                              ptr(A, f64p), K, ptr(XV, f64p), None))
    return XV


# ---- the arguments every entry shares ----------------------------------------------------------------------------------------
class _Scores:
    """a score matrix as the C ABI takes it: pointer, is_f32, on_device, leading dimension, rows, columns.  A host matrix
    is taken where it lies when its columns are contiguous (any leading dimension); anything else is copied once."""

    def __init__(self, pred, who, name="pred"):
        self.vector = False
        if isinstance(pred, DeviceArray):
            if pred.ptr is None:
                raise ValueError("%s: '%s' has been freed." % (who, name))
            self.keep, self.addr, self.f32, self.dev = pred, pred.ptr, 0, 1
            self.n, self.K, self.ld = pred.rows, pred.cols, pred.rows
        else:
            a = np.asarray(getattr(pred, "scores", pred))
            if a.dtype != np.float32:
                a = np.asarray(a, dtype=np.float64)
            if a.ndim == 1:
                self.vector = True
                a = a[:, None]
            if a.ndim != 2:
                raise ValueError("%s: '%s' should be a vector or a matrix." % (who, name))
            item = a.dtype.itemsize
            ok = a.shape[0] > 0 and a.shape[1] > 0 and a.strides[0] == item and a.strides[1] % item == 0 and \
                (a.shape[1] == 1 or a.strides[1] >= a.shape[0] * item)
            if not ok:
                a = np.asfortranarray(a)
            self.keep, self.addr, self.f32, self.dev = a, vp(a.ctypes.data), int(a.dtype == np.float32), 0
            self.n, self.K = a.shape
            self.ld = a.strides[1] // item if a.shape[1] > 1 and a.size else max(self.n, 1)
        if self.n < 1 or self.K < 1:
            raise ValueError("%s: '%s' should have at least one row and one column." % (who, name))
        if self.n > MAX_ROWS:
            raise ValueError("%s: 2^31 rows or more (the row indices are 32-bit)" % who)

    def first_nan_column(self, rows=None):
        """host matrices only: the first column with a NaN among the selected rows, or None"""
        if self.dev:
            return None
        a = self.keep if rows is None else self.keep[rows]
        bad = np.flatnonzero(np.isnan(a).any(axis=0))
        return int(bad[0]) if bad.size else None


def _target(target, n, who):
    t = np.asarray(target)
    if t.ndim != 1:
        t = np.ravel(t)
    if t.size != n:
        raise ValueError(ERROR_DIM + "\n'pred' and 'target' should have the same length.")
    with np.errstate(invalid="ignore"):
        ok = (t == 0) | (t == 1)
    if not np.all(ok):
        raise ValueError("%s: 'target' should hold 0 and 1 only (row %d holds %s)." % (who, int(np.flatnonzero(~ok)[0]), t[~ok][0]))
    y = np.ascontiguousarray(t, dtype=np.uint8)
    n1 = int(y.sum())
    if n1 == 0 or n1 == n:
        raise ValueError("%s: 'target' should hold both classes (it holds %d cases and %d controls)." % (who, n1, n - n1))
    return y


def _rows(ind_row, n_src, who):
    if ind_row is None:
        return None
    r = np.asarray(ind_row)
    if r.dtype == bool:
        r = np.flatnonzero(r)
    r = np.ascontiguousarray(r, dtype=np.int64)
    if r.ndim != 1 or r.size < 1:
        raise ValueError("%s: 'ind_row' should select at least one row." % who)
    if r.min() < 0 or r.max() >= n_src:
        raise ValueError("%s: 'ind_row' out of bounds (%d rows)." % (who, n_src))
    return r


NAN_MESSAGE = "%s: missing value (NaN) in 'pred', first in column %d."


def _auc(s, K, n_sum, target, ind_row, who):
    r = _rows(ind_row, s.n, who)
    n = s.n if r is None else r.size
    y = _target(target, n, who)
    if n_sum == 1:
        bad = s.first_nan_column(r)
        if bad is not None:
            raise ValueError(NAN_MESSAGE % (who, bad))
    out = np.empty(K)
    check(_lib.load().bsn_auc(s.addr, s.f32, s.dev, s.ld, s.n, K, n_sum, ptr(r, i64p), n, ptr(y, u8p), ptr(out, f64p)))
    return out


def AUC(pred, target, digits=None, ind_row=None):
    """bigstatsr::AUC for every column of `pred` at once: the probability that a case's score exceeds a control's, ties
    counting one half — twoU = 2 #{x_i > x_j} + #{x_i = x_j} over the pairs (case i, control j) in exact integers,
    AUC = twoU / (2 n1 n0).  `pred`: a vector (returns a float), an n x K host matrix (float32 or float64, any leading
    dimension) or a DeviceArray (returns K values); `target`: 0 / 1 per selected row, shared by all columns; `ind_row`:
    rows of `pred` to use.  -0.0 ties with +0.0, +-Inf are ordinary values; a NaN in `pred` is refused and the message
    names the first such column.  `digits` rounds on the host."""
    s = _Scores(pred, "AUC")
    out = _auc(s, s.K, 1, target, ind_row, "AUC")
    if digits is not None:
        out = np.round(out, int(digits))
    return float(out[0]) if s.vector else out


def snp_grid_AUC(multi_PRS, y_train, ind_row=None, n_chr=None):
    """`grid2$auc` of vignettes/SCT.Rmd ("Best C+T predictions"): the columns j, j + s, j + 2 s, ... of a snp_grid_PRS
    result hold the same grid row and threshold on successive chromosomes; they are summed on the device in fp64, in
    ascending chromosome order, and the AUC of every sum is taken.  Returns the table as a dict of arrays of length s: the
    columns of `all_keep.grid` (size, thr_r2, grp_num, thr_imp), `thr_lp`, `id` (the grid row, 0-based) and `auc`.
    `ind_row`: rows of the score matrix that `y_train` describes; `n_chr`: the number of chromosomes (default: the
    length of `multi_PRS.all_keep`)."""
    who = "snp_grid_AUC"
    all_keep = getattr(multi_PRS, "all_keep", None)
    if n_chr is None:
        if all_keep is None:
            raise ValueError("%s: 'n_chr' is needed for a plain matrix." % who)
        n_chr = len(all_keep)
    n_chr = int(n_chr)
    s = _Scores(multi_PRS, who, "multi_PRS")
    if n_chr < 1 or s.K % n_chr:
        raise ValueError("%s: the number of columns (%d) should be a multiple of the number of chromosomes (%d)." % (who, s.K, n_chr))
    width = s.K // n_chr
    auc = _auc(s, width, n_chr, y_train, ind_row, who)
    out = {}
    thr = getattr(multi_PRS, "grid_lpS_thr", None)
    grid = getattr(all_keep, "grid", None)
    if thr is not None and grid is not None:
        T = len(thr)
        n_grid = len(grid["size"])
        if n_grid * T != width:
            raise ValueError("%s: %d grid rows x %d thresholds do not give the %d columns of a chromosome." % (who, n_grid, T, width))
        for k in ("size", "thr_r2", "grp_num", "thr_imp"):
            out[k] = np.repeat(np.asarray(grid[k]), T)
        out["thr_lp"] = np.tile(np.asarray(thr, dtype=np.float64), n_grid)
        out["id"] = np.repeat(np.arange(n_grid), T)
    out["auc"] = auc
    return out


# ---- AUCBoot -------------------------------------------------------------------------------------------------------------
class BootAUC(np.ndarray):
    """K x 4 (4 values for a vector `pred`): Mean, 2.5%, 97.5% and Sd of the bootstrap replicates of the AUC.
    `.replicates`: nboot x K, NaN where a resample held one class only; `.seed`: the seed the draws came from;
    `.ms`: device milliseconds (auc_last_ms); `.names`: ("Mean", "2.5%", "97.5%", "Sd")."""
    replicates = seed = ms = None
    names = ("Mean", "2.5%", "97.5%", "Sd")

    def __array_finalize__(self, obj):
        if obj is not None:
            for a in ("replicates", "seed", "ms"):
                setattr(self, a, getattr(obj, a, None))


def boot_statistics(replicates):
    """Mean, the 2.5 % and 97.5 % quantiles (linear interpolation, R's type 7) and Sd (ddof = 1) of every column over
    the replicates that are not NaN: K x 4"""
    rep = np.asarray(replicates, dtype=np.float64)
    out = np.full((rep.shape[1], 4), np.nan)
    for j in range(rep.shape[1]):
        v = rep[:, j]
        v = v[~np.isnan(v)]
        if v.size:
            out[j, 0] = v.mean()
            out[j, 1:3] = np.quantile(v, [0.025, 0.975])
        if v.size > 1:
            out[j, 3] = v.std(ddof=1)
    return out


def AUCBoot(pred, target, nboot=10000, seed=None, digits=None):
    """bigstatsr::AUCBoot for every column of `pred`: `nboot` bootstrap replicates of the AUC on the device, then Mean,
    2.5%, 97.5% and Sd on the host (boot_statistics).  Replicate b draws n rows with replacement by the rule of
    csrc/auc_step.hpp from (b, seed) alone — R's sample() is not emulated — so every column of a call sees the same
    resamples and differences between models are paired.  `seed`: an integer below 2^64 (default: drawn from the
    system, reported in `.seed`).  Returns a BootAUC."""
    who = "AUCBoot"
    s = _Scores(pred, who)
    y = _target(target, s.n, who)
    nboot = int(nboot)
    if not 1 <= nboot <= MAX_ROWS:
        raise ValueError("%s: 'nboot' should be between 1 and 2^31 - 1." % who)
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("%s: 'seed' should be between 0 and 2^64 - 1." % who)
    bad = s.first_nan_column()
    if bad is not None:
        raise ValueError(NAN_MESSAGE % (who, bad))
    rep = np.empty((nboot, s.K), order="F")
    check(_lib.load().bsn_auc_boot(s.addr, s.f32, s.dev, s.ld, s.n, s.K, ptr(y, u8p), nboot, C.c_uint64(seed), ptr(rep, f64p)))
    st = boot_statistics(rep)
    if digits is not None:
        st = np.round(st, int(digits))
    out = (st[0] if s.vector else st).view(BootAUC)
    out.replicates, out.seed, out.ms = rep, seed, auc_last_ms()
    return out


def auc_boot_draws(n, b, seed):
    """the n rows that replicate `b` of an AUCBoot call with `seed` draws, generated on the device (bsn_auc_boot_draws)"""
    rows = np.empty(int(n), dtype=np.int32)
    check(_lib.load().bsn_auc_boot_draws(int(n), int(b), C.c_uint64(int(seed)), ptr(rows, i32p)))
    return rows


# ---- pcor ----------------------------------------------------------------------------------------------------------------
def pcor(x, y, z=None, alpha=0.05):
    """bigstatsr::pcor for every column of `x`: the partial correlation with `y` given [1, z] and its Fisher interval,
    K x 3 (3 values for a vector): r = cor(resid(x ~ 1 + z), resid(y ~ 1 + z)), bounds
    tanh(atanh(r) +- qnorm(1 - alpha / 2) / sqrt(n - c - 3)) with c the number of columns of `z`.  The host takes the thin
    QR of [1, z] and the residual r_y; the device makes two passes over `x` (a = Q'x, then e = x - Q a with e'e and
    e'r_y): the residual form, so a score whose mean dwarfs its spread loses nothing.  `x`: a vector, a host matrix or a
    DeviceArray.  A constant column of `x` gives NaN."""
    who = "pcor"
    s = _Scores(x, who, "x")
    n = s.n
    yv = np.ascontiguousarray(np.ravel(np.asarray(y)), dtype=np.float64)
    if yv.size != n:
        raise ValueError(ERROR_DIM + "\n'x' and 'y' should have the same length.")
    Z = np.ones((n, 1))
    if z is not None:
        zz = np.asarray(getattr(z, "values", z), dtype=np.float64)
        if zz.ndim == 1:
            zz = zz[:, None]
        if zz.ndim != 2 or zz.shape[0] != n:
            raise ValueError(ERROR_DIM + "\n'x' and 'z' should have the same number of rows.")
        Z = np.hstack([Z, zz])
    p = Z.shape[1]
    c = p - 1
    if p > MAX_COVAR:
        raise ValueError("%s: [1, z] should have at most %d columns (got %d)." % (who, MAX_COVAR, p))
    if not (0 < alpha < 1):
        raise ValueError("%s: 'alpha' should be between 0 and 1." % who)
    if not (np.isfinite(yv).all() and np.isfinite(Z).all()) or (not s.dev and not np.isfinite(s.keep).all()):
        raise ValueError("%s: non-finite value (NA, NaN or Inf) in the input." % who)
    if n - c - 3 <= 0:
        raise ValueError("%s: too few rows: n - c - 3 = %d should be positive." % (who, n - c - 3))
    Q, R = np.linalg.qr(Z)
    d = np.abs(np.diag(R))
    if d.min() <= d.max() * max(n, p) * np.finfo(np.float64).eps:
        raise ValueError("%s: [1, z] is rank-deficient." % who)
    Q = np.asfortranarray(Q)
    ry = yv - Q @ (Q.T @ yv)
    ry = np.ascontiguousarray(ry - Q @ (Q.T @ ry))       # a second sweep: r_y is orthogonal to Q to the last place
    ee, ery = np.empty(s.K), np.empty(s.K)
    check(_lib.load().bsn_pcor_moments(s.addr, s.f32, s.dev, s.ld, n, s.K, ptr(Q, f64p), p, ptr(ry, f64p), ptr(ee, f64p), ptr(ery, f64p)))
    if not np.isfinite(ee).all():
        raise ValueError("%s: non-finite value (NA, NaN or Inf) in the input." % who)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = ery / np.sqrt(ee * float(ry @ ry))
    r = np.clip(r, -1.0, 1.0)
    q = NormalDist().inv_cdf(1.0 - alpha / 2.0) / np.sqrt(n - c - 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.arctanh(r)
        out = np.column_stack([r, np.tanh(f - q), np.tanh(f + q)])
    return out[0] if s.vector else out
