"""LD scores, LD score regression, LDpred2-inf and LDpred2-grid over the resident SFBM — host mirror of R/ldsc.R,
R/LDpred2.R:27-140 and of bigsparser's sp_prodVec / sp_solve_sym.

The sparse products run on the device (bsn_sfbm_prodvec, bsn_sfbm_ld_scores, bsn_sfbm_solve_sym), and so do the Gibbs
chains of snp_ldpred2_grid (bsn_ldpred2_gibbs); the regression itself works on vectors of length M and is numpy on the
host, as it is R in the reference.  Indices are 0-based.  Every device sum has a fixed order: two calls on the same
inputs (and, for the sampler, the same seed) return the same bits."""
import ctypes as C
import os
from statistics import NormalDist

import numpy as np

from . import _lib
from ._lib import as_f64, check, f64p, i32p, i64p, ptr, u64p
from .bed import ERROR_DIM
from .lassosum2 import SFBM, _col, _ncol, as_SFBM

ERROR_LENGTH = ERROR_DIM + "\nArguments should have the same length."


class SolveResult(np.ndarray):
    """the solution of sp_solve_sym; `.iters` MINRES iterations, `.relres` the true ||b - (A + D) x|| / ||b||"""
    iters = None
    relres = None

    def __array_finalize__(self, obj):
        if obj is not None:
            self.iters = getattr(obj, "iters", None)
            self.relres = getattr(obj, "relres", None)


def _subset(corr, ind, n, name, repeats_ok=False):
    """the checks on an index vector, before any device work; None when it selects every column in order"""
    m2 = _ncol(corr)
    if ind is None:
        if n is not None and n != m2:
            raise ValueError(ERROR_LENGTH)
        return None
    ind = np.ascontiguousarray(np.ravel(ind), dtype=np.int64)
    if n is not None and ind.size != n:
        raise ValueError(ERROR_LENGTH)
    if not np.all((ind >= 0) & (ind < m2)):
        raise ValueError("all(%s %%in%% cols_along(corr)) is not TRUE" % name)
    if not repeats_ok and np.unique(ind).size != ind.size:
        raise ValueError("'%s' should not have repeated indices." % name)
    return ind


class _Resident:
    """corr as an SFBM for the length of one call: converted (and freed again) only when it is not one already"""

    def __init__(self, corr):
        self.own = not isinstance(corr, SFBM)
        self.corr = corr

    def __enter__(self):
        self.sf = as_SFBM(self.corr)
        return self.sf

    def __exit__(self, *exc):
        if self.own:
            self.sf.close()


def sp_prodVec(corr, x, ind_corr=None):
    """bigsparser::sp_prodVec on corr[ind_corr, ind_corr] (all of corr by default): corr . x.  A repeated index is refused."""
    x = as_f64(np.ravel(np.asarray(x, dtype=np.float64)))
    ind = _subset(corr, ind_corr, x.size, "ind.corr")
    with _Resident(corr) as sf:
        y = np.empty(x.size, dtype=np.float64)
        check(_lib.load().bsn_sfbm_prodvec(sf.handle, ptr(x, f64p), ptr(ind, i64p), x.size, ptr(y, f64p)))
    return y


sp_cprodVec = sp_prodVec   # the matrix is symmetric


def ld_scores_sfbm(corr, ind_sub=None):
    """src/ld-scores-sfbm.cpp:10-69: for each listed column, the sum of x^2 over its stored entries whose row is listed too
    (all columns by default).  The list is a mask: a repeated index gives a repeated value."""
    ind = _subset(corr, ind_sub, None, "ind_sub", repeats_ok=True)
    with _Resident(corr) as sf:
        m = sf.ncol if ind is None else ind.size
        out = np.empty(m, dtype=np.float64)
        check(_lib.load().bsn_sfbm_ld_scores(sf.handle, ptr(ind, i64p), m, ptr(out, f64p)))
    return out


def sp_colSumsSq_sym(p, i, x):
    """src/sp-colsumssq-sym.cpp:9-32: colSums(A^2) of a symmetric matrix given as the CSC of its upper triangle"""
    p = np.asarray(p)
    with SFBM(p, i, x, p.size - 1, upper=True) as sf:
        return ld_scores_sfbm(sf)


def sp_solve_sym(corr, b, add_to_diag=0, tol=1e-10, maxiter=None, ind_corr=None):
    """Solves (corr[ind_corr, ind_corr] + diag(add_to_diag)) x = b (bigsparser::sp_solve_sym) by MINRES on the device.  The
    iteration stops on the recurrence's residual, the true residual ||b - (A + D) x|| / ||b|| is then formed with one more
    product and has to be <= tol; BsnError (naming the iterations and the residual reached) after maxiter iterations
    without that.  tol = 1e-10 and maxiter = 10 * length(b) are this project's choice.  Returns x with `.iters` and
    `.relres`."""
    b = as_f64(np.ravel(np.asarray(b, dtype=np.float64)))
    m = b.size
    ind = _subset(corr, ind_corr, m, "ind.corr")
    d = np.asarray(add_to_diag, dtype=np.float64)
    if d.ndim == 0 or d.size == 1:
        d = np.full(m, float(d.ravel()[0]) if d.size else 0.0)
    d = as_f64(np.ravel(d))
    if d.size != m:
        raise ValueError(ERROR_LENGTH)
    if not tol > 0:
        raise ValueError("'tol' should have only positive values.")
    maxiter = 10 * max(m, 1) if maxiter is None else int(maxiter)
    if maxiter < 1:
        raise ValueError("'maxiter' should be at least 1.")
    with _Resident(corr) as sf:
        x = np.empty(m, dtype=np.float64)
        iters, relres = C.c_int32(0), C.c_double(0.0)
        check(_lib.load().bsn_sfbm_solve_sym(sf.handle, ptr(b, f64p), ptr(d, f64p), ptr(ind, i64p), m, float(tol),
                                             min(maxiter, 2 ** 31 - 1), ptr(x, f64p), C.byref(iters), C.byref(relres)))
    out = x.view(SolveResult)
    out.iters, out.relres = int(iters.value), float(relres.value)
    return out


def _sumstats(df_beta):
    """assert_df_with_names(df_beta, c("beta", "beta_se", "n_eff")); a single n_eff is recycled as a data frame does"""
    beta, beta_se, n_eff = (_col(df_beta, n) for n in ("beta", "beta_se", "n_eff"))
    if n_eff.size == 1:
        n_eff = np.repeat(n_eff, beta.size)
    return beta, beta_se, n_eff


# ---- R/ldsc.R ----------------------------------------------------------------------------------------------------------

def WEIGHTS(pred, w_ld):
    """heteroscedasticity and overcounting weights (R/ldsc.R:4-6)"""
    return 1 / (pred ** 2 * w_ld)


def wlm(x, y, w):
    """R/ldsc.R:11-21, equivalent to stats::lm.wfit(cbind(1, x), y, w): (intercept, slope, pred)"""
    wx = w * x
    W, WX = np.sum(w), np.sum(wx)
    WY, WXX, WXY = np.dot(w, y), np.dot(wx, x), np.dot(wx, y)
    alpha = (WXX * WY - WX * WXY) / (W * WXX - WX ** 2)
    beta = (WXY * W - WX * WY) / (W * WXX - WX ** 2)
    return alpha, beta, x * beta + alpha


def wlm_no_int(x, y, w):
    """R/ldsc.R:24-30, equivalent to stats::lm.wfit(as.matrix(x), y, w): (slope, pred)"""
    wx = w * x
    beta = np.dot(wx, y) / np.dot(wx, x)
    return beta, x * beta


def _ldsc_two_step(ld_score, ld_size, chi2, sample_size, intercept, chi2_thr1, chi2_thr2):
    """R/ldsc.R:85-122 (blocks = NULL), chi2 already shifted"""
    if intercept is None:
        sub1 = chi2 < chi2_thr1
        w_ld = np.maximum(ld_score[sub1], 1)
        x1 = (ld_score / ld_size * sample_size)[sub1]
        y1 = chi2[sub1]
        pred0 = y1
        for _ in range(100):
            pred = wlm(x1, y1, WEIGHTS(pred0, w_ld))[2]
            if np.max(np.abs(pred - pred0)) < 1e-6:
                break
            pred0 = pred
        step1_int = wlm(x1, y1, WEIGHTS(pred0, w_ld))[0]
    else:
        step1_int = intercept
    sub2 = chi2 < chi2_thr2
    w_ld = np.maximum(ld_score[sub2], 1)
    x = (ld_score / ld_size * sample_size)[sub2]
    y = chi2[sub2]
    yp = y - step1_int
    pred0 = y
    for _ in range(100):
        pred = step1_int + wlm_no_int(x, yp, WEIGHTS(pred0, w_ld))[1]
        if np.max(np.abs(pred - pred0)) < 1e-6:
            break
        pred0 = pred
    step2_h2 = wlm_no_int(x, yp, WEIGHTS(pred0, w_ld))[0]
    return step1_int, step2_h2


def snp_ldsc(ld_score, ld_size, chi2, sample_size, blocks=200, intercept=None, chi2_thr1=30, chi2_thr2=np.inf, ncores=1):
    """R/ldsc.R:66-158.  Returns a dict with int, int_se, h2, h2_se (int and h2 only when blocks is None).  ncores is
    accepted for the reference's signature; the jackknife runs on the host, one block after the other."""
    chi2 = np.ravel(np.asarray(chi2, dtype=np.float64)) + 1e-8
    ld_score = np.ravel(np.asarray(ld_score, dtype=np.float64))
    if not np.all(chi2 > 0):
        raise ValueError("'chi2' should have only positive values.")
    if chi2.size != ld_score.size:
        raise ValueError(ERROR_LENGTH)
    if np.size(ld_size) != 1:
        raise ValueError(ERROR_LENGTH)
    ld_size = np.ravel(ld_size)[0]
    if ld_size != np.trunc(ld_size):
        raise ValueError("'ld_size' should contain only integers.")
    ld_size = float(ld_size)
    if not (int(ncores) == ncores and ncores >= 1):
        raise ValueError("'ncores' should be an integer >= 1.")
    M = chi2.size
    sample_size = np.ravel(np.asarray(sample_size, dtype=np.float64))
    if sample_size.size == 1:
        sample_size = np.repeat(sample_size, M)
    elif sample_size.size != M:
        raise ValueError(ERROR_LENGTH)
    intercept = None if intercept is None else float(intercept)

    if blocks is None:
        a, h2 = _ldsc_two_step(ld_score, ld_size, chi2, sample_size, intercept, chi2_thr1, chi2_thr2)
        return {"int": float(a), "h2": float(h2)}

    # delete-a-group jackknife variance estimator (R/ldsc.R:126-155)
    if np.size(blocks) == 1:
        nb = int(np.ravel(blocks)[0])
        blocks = np.sort(np.resize(np.arange(1, nb + 1), M))    # sort(rep_len(seq_len(blocks), M))
    else:
        blocks = np.ravel(np.asarray(blocks))
        if blocks.size != M:
            raise ValueError(ERROR_LENGTH)
    groups = [np.nonzero(blocks == g)[0] for g in np.unique(blocks)]      # split(seq_along(blocks), blocks)
    h_blocks = M / np.array([g.size for g in groups], dtype=np.float64)

    def delete(ind_rm):
        keep = np.ones(M, dtype=bool)
        if ind_rm is not None:
            keep[ind_rm] = False
        # the reference calls itself here with the shifted chi2, which is shifted once more (R/ldsc.R:73, :140)
        return _ldsc_two_step(ld_score[keep], ld_size, chi2[keep] + 1e-8, sample_size[keep], intercept, chi2_thr1, chi2_thr2)

    estim = delete(None)
    del_int, del_h2 = (np.array(v, dtype=np.float64) for v in zip(*[delete(g) for g in groups]))
    # https://doi.org/10.1023/A:1008800423698
    int_pseudo = h_blocks * estim[0] - (h_blocks - 1) * del_int
    h2_pseudo = h_blocks * estim[1] - (h_blocks - 1) * del_h2
    int_J = np.sum(int_pseudo / h_blocks)
    h2_J = np.sum(h2_pseudo / h_blocks)
    return {"int": float(int_J),
            "int_se": float(np.sqrt(np.mean((int_pseudo - int_J) ** 2 / (h_blocks - 1)))),
            "h2": float(h2_J),
            "h2_se": float(np.sqrt(np.mean((h2_pseudo - h2_J) ** 2 / (h_blocks - 1))))}


def snp_ldsc2(corr, df_beta, blocks=None, intercept=1, ncores=1, ind_beta=None, chi2_thr1=30, chi2_thr2=np.inf):
    """R/ldsc.R:192-224: the LD scores of every column of corr on the device (ld_scores_sfbm), then snp_ldsc on
    full_ld[ind_beta] with ld_size = ncol(corr).  corr: an SFBM or anything as_SFBM takes (converted for this call only)."""
    beta, beta_se, n_eff = _sumstats(df_beta)
    m2 = _ncol(corr)
    ind = np.arange(m2, dtype=np.int64) if ind_beta is None else np.ascontiguousarray(np.ravel(ind_beta), dtype=np.int64)
    if ind.size != beta.size:
        raise ValueError(ERROR_LENGTH)
    if not np.all((ind >= 0) & (ind < m2)):
        raise ValueError("all(ind.beta %in% cols_along(corr)) is not TRUE")
    if not np.all(beta_se > 0):
        raise ValueError("'df_beta$beta_se' should have only positive values.")
    if not (beta.size == beta_se.size == n_eff.size):
        raise ValueError(ERROR_LENGTH)
    full_ld = ld_scores_sfbm(corr)
    return snp_ldsc(full_ld[ind], m2, (beta / beta_se) ** 2, n_eff, blocks=blocks, intercept=intercept, ncores=ncores,
                    chi2_thr1=chi2_thr1, chi2_thr2=chi2_thr2)


def coef_to_liab(K_pop, K_gwas=0.5):
    """R/ldsc.R:245-250: coefficient to convert e.g. a heritability to the liability scale"""
    nd = NormalDist()
    z = nd.pdf(nd.inv_cdf(min(K_pop, 1 - K_pop)))
    return (K_pop * (1 - K_pop) / z) ** 2 / (K_gwas * (1 - K_gwas))


# ---- R/LDpred2.R:27-42 ---------------------------------------------------------------------------------------------------

def snp_ldpred2_inf(corr, df_beta, h2):
    """R/LDpred2.R:27-42: effects under the infinitesimal model, (corr + diag(ncol(corr) / (h2 N))) x = beta_hat solved on
    the device (sp_solve_sym with its default tol and maxiter) and scaled back.  corr: an SFBM or anything as_SFBM takes."""
    beta, beta_se, n_eff = _sumstats(df_beta)
    m2 = _ncol(corr)
    if not (m2 == beta.size == beta_se.size == n_eff.size):
        raise ValueError(ERROR_LENGTH)
    if not np.all(beta_se > 0):
        raise ValueError("'df_beta$beta_se' should have only positive values.")
    if not np.all(np.asarray(h2, dtype=np.float64) > 0):
        raise ValueError("'h2' should have only positive values.")
    N = n_eff
    scale = np.sqrt(N * beta_se ** 2 + beta ** 2)
    beta_hat = beta / scale
    beta_inf = sp_solve_sym(corr, beta_hat, add_to_diag=m2 / (float(h2) * N))
    return np.asarray(beta_inf) * scale


# ---- R/LDpred2.R:73-140 --------------------------------------------------------------------------------------------------

class LDpred2Grid(np.ndarray):
    """beta_grid (m x number of chains; m x num_iter with return_sampling_betas).  `.seed` is the key the random numbers
    of the call came from (the same seed gives the same bits), `.grid_param` holds p, h2, sparse, stream and `time`,
    each chain's seconds on the device clock (all chains of a call run at the same time)."""
    seed = None
    grid_param = None

    def __array_finalize__(self, obj):
        if obj is not None:
            self.seed = getattr(obj, "seed", None)
            self.grid_param = getattr(obj, "grid_param", None)


def _grid_col(grid_param, name, dtype):
    try:
        has = name in grid_param
    except TypeError:
        has = False
    if not has:
        raise ValueError("'grid_param' should have element '%s'." % name)
    return np.ascontiguousarray(np.ravel(np.asarray(grid_param[name])), dtype=dtype)


def snp_ldpred2_grid(corr, df_beta, grid_param, burn_in=50, num_iter=100, ncores=1, return_sampling_betas=False,
                     ind_corr=None, seed=None):
    """R/LDpred2.R:73-140: one Gibbs chain per row of grid_param (a mapping or DataFrame with p, h2, sparse), all of them
    in one library call over the resident matrix.  corr: an SFBM or anything as_SFBM takes (converted for this call
    only).  Returns an LDpred2Grid: m x nrow(grid_param), NaN columns where the reference returns NA; with
    return_sampling_betas (one row of grid_param only) m x num_iter, the effects after each sweep past burn-in.

    The random numbers.  R's generator cannot be reproduced; U and Z of (chain, sweep, position in ind_corr) come from
    a counter-based generator keyed by `seed`.  seed=None draws a fresh seed, so two calls differ, as in the reference
    without set.seed; the seed used is kept on the result.  A chain's stream id is its row in grid_param unless
    grid_param has an element 'stream': a chain's result depends on (seed, stream, its own parameters) alone, not on
    the other rows or their order.  ncores is accepted for the reference's signature."""
    # the reference's checks, in its order, before any device work
    beta, beta_se, n_eff = _sumstats(df_beta)
    pp, h2 = (_grid_col(grid_param, n, np.float64) for n in ("p", "h2"))
    sparse = _grid_col(grid_param, "sparse", bool).astype(np.int32)
    ind = _subset(corr, ind_corr, beta.size, "ind.corr", repeats_ok=True)
    if not np.all(beta_se > 0):
        raise ValueError("'df_beta$beta_se' should have only positive values.")
    if not np.all(h2 > 0):
        raise ValueError("'grid_param$h2' should have only positive values.")
    if not (int(ncores) == ncores and ncores >= 1):
        raise ValueError("'ncores' should be an integer >= 1.")
    if not (beta.size == beta_se.size == n_eff.size) or not (pp.size == h2.size == sparse.size):
        raise ValueError(ERROR_LENGTH)
    G = pp.size
    if return_sampling_betas and G != 1:
        raise ValueError("Only one set of parameters is allowed when using 'return_sampling_betas'.")
    if ind is not None and np.unique(ind).size != ind.size:
        raise ValueError("'ind.corr' should not have repeated indices.")
    has_stream = False
    try:
        has_stream = "stream" in grid_param
    except TypeError:
        pass
    stream = _grid_col(grid_param, "stream", np.uint64) if has_stream else np.arange(G, dtype=np.uint64)
    if stream.size != G:
        raise ValueError(ERROR_LENGTH)
    burn_in, num_iter = int(burn_in), int(num_iter)
    if burn_in < 0:
        raise ValueError("'burn_in' should not be negative.")
    if num_iter < 1:
        raise ValueError("'num_iter' should be at least 1.")
    seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & (2 ** 64 - 1)

    N = n_eff
    scale = np.sqrt(N * beta_se ** 2 + beta ** 2)
    beta_hat = as_f64(beta / scale)
    N = as_f64(N)
    m = beta_hat.size
    secs = np.zeros(G)
    L = _lib.load()
    with _Resident(corr) as sf:
        if return_sampling_betas:
            out = np.empty((m, num_iter), dtype=np.float64, order="F")
            check(L.bsn_ldpred2_gibbs_sampling(sf.handle, ptr(beta_hat, f64p), ptr(N, f64p), m, ptr(ind, i64p), float(h2[0]),
                                               float(pp[0]), int(sparse[0]), int(stream[0]), burn_in, num_iter, seed,
                                               out.ctypes.data_as(f64p), secs.ctypes.data_as(f64p)))
        else:
            out = np.empty((m, G), dtype=np.float64, order="F")
            check(L.bsn_ldpred2_gibbs(sf.handle, ptr(beta_hat, f64p), ptr(N, f64p), m, ptr(ind, i64p), ptr(h2, f64p),
                                      ptr(pp, f64p), ptr(sparse, i32p), ptr(stream, u64p), G, burn_in, num_iter, seed,
                                      out.ctypes.data_as(f64p), secs.ctypes.data_as(f64p)))
    res = (out * scale[:, None]).view(LDpred2Grid)      # sweep(beta_gibbs, 1, scale, '*')
    res.seed = seed
    res.grid_param = {"p": pp, "h2": h2, "sparse": sparse.astype(bool), "stream": stream, "time": secs}
    return res


# ---- R/LDpred2.R:203-286 -------------------------------------------------------------------------------------------------

def snp_ldpred2_auto(corr, df_beta, h2_init, vec_p_init=0.1, burn_in=500, num_iter=200, sparse=False, verbose=False,
                     report_step=None, allow_jump_sign=True, shrink_corr=1, use_MLE=True, p_bounds=(1e-5, 1),
                     alpha_bounds=(-1.5, 0.5), ind_corr=None, ncores=1, seed=None, stream=None):
    """R/LDpred2.R:203-286: one LDpred2-auto chain per value of vec_p_init, all of them in one library call over the
    resident matrix (bsn_ldpred2_auto).  corr: an SFBM or anything as_SFBM takes (converted for this call only).
    Returns a list of dicts in the order of vec_p_init with the reference's elements — beta_est (scaled back), postp_est,
    corr_est, sample_beta (dense m x (num_iter // report_step); report_step=None is the reference's num_iter + 1, no
    column), path_p_est, path_h2_est, path_alpha_est, h2_est, p_est, alpha_est (means over the last num_iter sweeps),
    h2_init, p_init — and seed, stream, time (the chain's seconds on the device clock).  A chain that diverged has NaN
    estimates, as the reference has NA.  sparse=True adds beta_est_sparse to every chain whose h2_est is finite: one
    further bsn_ldpred2_gibbs call (sparse, burn-in 50, 100 sweeps) at each chain's h2_est and p_est, made through
    snp_ldpred2_grid: beta_est_sparse is bit for bit what that function returns for the chain by hand.

    The random numbers come from the counter-based generator of snp_ldpred2_grid, keyed by `seed` (None: a fresh one,
    kept on the result); a chain's stream id is its position in vec_p_init unless `stream` gives it, and must be below
    2^63: the sparse follow-up runs at stream | 2^63 and so reuses no counter.  The MLE of (alpha, sigma2) is the exact
    minimiser over the reference's box, not an L-BFGS-B run.  verbose and ncores are accepted
    for the reference's signature."""
    # the reference's checks, in its order, before any device work
    beta, beta_se, n_eff = _sumstats(df_beta)
    ind = _subset(corr, ind_corr, beta.size, "ind.corr", repeats_ok=True)
    if not np.all(beta_se > 0):
        raise ValueError("'df_beta$beta_se' should have only positive values.")
    if not np.all(np.asarray(h2_init, dtype=np.float64) > 0) or np.size(h2_init) != 1:
        raise ValueError("'h2_init' should have only positive values.")
    if not (int(ncores) == ncores and ncores >= 1):
        raise ValueError("'ncores' should be an integer >= 1.")
    if not (beta.size == beta_se.size == n_eff.size):
        raise ValueError(ERROR_LENGTH)
    if ind is not None and np.unique(ind).size != ind.size:
        raise ValueError("'ind.corr' should not have repeated indices.")
    p_init = as_f64(np.ravel(np.asarray(vec_p_init, dtype=np.float64)))
    G = p_init.size
    if np.any(np.isnan(p_init)):
        raise ValueError("'vec_p_init' should not have missing values.")
    burn_in, num_iter = int(burn_in), int(num_iter)
    if burn_in < 0:
        raise ValueError("'burn_in' should not be negative.")
    if num_iter < 1:
        raise ValueError("'num_iter' should be at least 1.")
    if burn_in + num_iter >= 2 ** 30:
        raise ValueError("'burn_in + num_iter' should be below 2^30.")
    report_step = num_iter + 1 if report_step is None else int(report_step)
    if report_step < 1:
        raise ValueError("'report_step' should be at least 1.")
    report_step = min(report_step, num_iter + 1)
    p_lo, p_hi = (float(v) for v in p_bounds)
    a_lo, a_hi = (float(v) + 1 for v in alpha_bounds)      # alpha_bounds + 1 (R/LDpred2.R:254)
    if not (0 < p_lo <= p_hi <= 1):
        raise ValueError("'p_bounds' should be ordered and in (0, 1].")
    if not a_lo <= a_hi:
        raise ValueError("'alpha_bounds' should be ordered.")
    if stream is None:
        stream = np.arange(G, dtype=np.uint64)
    else:
        stream = np.ravel(np.asarray(stream))
        if stream.size != G:
            raise ValueError(ERROR_LENGTH)
        if np.any(stream < 0) or np.any(stream.astype(np.uint64) >= np.uint64(2 ** 63)):
            raise ValueError("'stream' should be in [0, 2^63).")
        stream = np.ascontiguousarray(stream, dtype=np.uint64)
    seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & (2 ** 64 - 1)
    h2_init = float(np.ravel(h2_init)[0])

    N = as_f64(n_eff)
    sd = 1 / np.sqrt(N * beta_se ** 2 + beta ** 2)
    beta_hat = as_f64(beta * sd)
    log_var = as_f64(2 * np.log(sd))
    m = beta_hat.size
    tot = burn_in + num_iter
    n_report = num_iter // report_step
    beta_est, postp_est, corr_est = (np.empty((m, G), dtype=np.float64, order="F") for _ in range(3))
    sample = np.empty((m, n_report, G), dtype=np.float64, order="F")
    path_p, path_h2, path_alpha = (np.empty((tot, G), dtype=np.float64, order="F") for _ in range(3))
    secs = np.zeros(G)
    beta_sparse = None
    L = _lib.load()
    with _Resident(corr) as sf:
        mean_ld = float(np.mean(ld_scores_sfbm(sf, ind)))
        check(L.bsn_ldpred2_auto(sf.handle, ptr(beta_hat, f64p), ptr(N, f64p), ptr(log_var, f64p), m, ptr(ind, i64p),
                                 ptr(p_init, f64p), ptr(stream, u64p), G, h2_init, burn_in, num_iter, report_step,
                                 int(not allow_jump_sign), float(shrink_corr), int(bool(use_MLE)), p_lo, p_hi, a_lo, a_hi,
                                 mean_ld, seed, beta_est.ctypes.data_as(f64p), postp_est.ctypes.data_as(f64p),
                                 corr_est.ctypes.data_as(f64p), sample.ctypes.data_as(f64p), path_p.ctypes.data_as(f64p),
                                 path_h2.ctypes.data_as(f64p), path_alpha.ctypes.data_as(f64p), secs.ctypes.data_as(f64p)))
        h2_est = np.array([np.mean(path_h2[burn_in:, g]) for g in range(G)])
        p_est = np.array([np.mean(path_p[burn_in:, g]) for g in range(G)])
        alpha_est = np.array([np.mean(path_alpha[burn_in:, g]) for g in range(G)])
        ok = np.nonzero(np.isfinite(h2_est))[0]      # sparse && !is.na(h2_est)
        if sparse and ok.size:
            # ldpred2_gibbs_one through snp_ldpred2_grid, so that the result is what that call gives by hand, bit for bit (it
            # forms beta_hat as beta / sqrt(...) and scales back by the product; the reference's beta * sd and / sd here
            # differ from that in the last place)
            gp = {"p": p_est[ok], "h2": h2_est[ok], "sparse": np.ones(ok.size, dtype=bool),
                  "stream": np.ascontiguousarray(stream[ok] | np.uint64(2 ** 63))}
            beta_sparse = np.asarray(snp_ldpred2_grid(sf, {"beta": beta, "beta_se": beta_se, "n_eff": n_eff}, gp, burn_in=50,
                                                      num_iter=100, ind_corr=ind, seed=seed))
    out = []
    for g in range(G):
        r = {"beta_est": beta_est[:, g] / sd, "postp_est": postp_est[:, g].copy(), "corr_est": corr_est[:, g].copy(),
             "sample_beta": np.ascontiguousarray(sample[:, :, g]), "path_p_est": path_p[:, g].copy(),
             "path_h2_est": path_h2[:, g].copy(), "path_alpha_est": path_alpha[:, g].copy(),
             "h2_est": float(h2_est[g]), "p_est": float(p_est[g]), "alpha_est": float(alpha_est[g]),
             "h2_init": h2_init, "p_init": float(p_init[g]), "seed": seed, "stream": int(stream[g]), "time": float(secs[g])}
        if beta_sparse is not None and g in ok:
            r["beta_est_sparse"] = beta_sparse[:, int(np.nonzero(ok == g)[0][0])].copy()
        out.append(r)
    return out
