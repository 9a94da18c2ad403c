"""big_univLinReg / big_univLogReg — host mirror of bigstatsr's per-variant association scans (external to the reference
tree like big_randomSVD; tests/testthat/test-6-PRS.R:19-22 calls the logistic one).  Indices are 0-based.

bsn_univ_linreg: one crossproduct pass over the panel [y~, U] plus the exact code counts, then k_ulr_final.
bsn_univ_logreg: k_logreg (bigsnpr_amd/csrc/gwas.hip), the per-variant iteratively reweighted least squares in fp64 with
the weighted Gram matrices on the f64 MFMA; the covariates-only model is fitted inside the library.

What differs from bigstatsr: a variant whose fit has not converged after `maxiter` solves keeps its last iterate and
niter = -1 (bigstatsr refits it with glm; that is not emulated here), and a variant with a missing value among
`ind_train` is NaN in every output (bigstatsr has no missing-value handling and returns NA)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BsnError, check, f64p, i64p, ptr
from .ld import _ind

MAX_COVAR = 30   # with the intercept and the variant: 32 columns


def _covar(covar_train, n):
    if covar_train is None:
        return np.empty((n, 0), order="F")
    cov = np.asarray(covar_train, dtype=np.float64)
    if cov.ndim == 1:
        cov = cov[:, None]
    if cov.ndim != 2 or cov.shape[0] != n:
        raise BsnError("Incompatibility between dimensions.\n'covar.train' and 'ind.train' should have the same length.")
    if cov.shape[1] > MAX_COVAR:
        raise BsnError("'covar.train' has more than %d columns." % MAX_COVAR)
    if not np.all(np.isfinite(cov)):
        raise BsnError("You can't have missing values in 'covar.train'.")
    return np.asfortranarray(cov)


def _train(G, ind_train, ind_col):
    """(rows, thunk): the thunk returns (image, rows, columns); the image is looked at last, so that the argument checks
    need no device"""
    if ind_train is None:
        ir = np.arange(G.nrow, dtype=np.int64)
    else:
        ir = np.ascontiguousarray(ind_train, dtype=np.int64).ravel()
    return ir, lambda: _ind(G, ir, ind_col)


def _y(y_train, n, name):
    y = np.ascontiguousarray(y_train, dtype=np.float64).ravel()
    if y.size != n:
        raise BsnError("Incompatibility between dimensions.\n'%s' and 'ind.train' should have the same length." % name)
    if not np.all(np.isfinite(y)):
        raise BsnError("You can't have missing values in '%s'." % name)
    return y


def covar_basis(covar, thr_eigval=1e-4):
    """U: the left singular vectors of [1, covar] whose singular value d has d / sqrt(n) > thr_eigval"""
    n = covar.shape[0]
    u, d, _ = np.linalg.svd(np.column_stack([np.ones(n), covar]), full_matrices=False)
    keep = d / np.sqrt(n) > thr_eigval
    return np.asfortranarray(u[:, keep])


def big_univLinReg(G, y_train, ind_train=None, ind_col=None, covar_train=None, thr_eigval=1e-4):
    """bigstatsr::big_univLinReg: per variant, the slope of y ~ x + 1 + covar, its standard error and t-score."""
    ir, image = _train(G, ind_train, ind_col)
    n = ir.size
    y = _y(y_train, n, "y.train")
    U = covar_basis(_covar(covar_train, n), thr_eigval)
    K = U.shape[1]
    if n - K - 1 <= 0:
        raise BsnError("big_univLinReg: no degrees of freedom left (n = %d, K = %d)." % (n, K))
    im, ir, ic = image()
    estim, se = np.empty(ic.size), np.empty(ic.size)
    check(_lib.load().bsn_univ_linreg(im.handle, ptr(ir, i64p), n, ptr(ic, i64p), ic.size, ptr(y, f64p),
                                      U.ctypes.data_as(f64p), K, ptr(estim, f64p), ptr(se, f64p)))
    score, df = estim / se, n - K - 1

    def predict(log10=True):
        from scipy.stats import t
        lp = (np.log(2.0) + t.logsf(np.abs(score), df)) / np.log(10)
        return lp if log10 else 10.0 ** lp
    return dict(estim=estim, std_err=se, score=score, df=df, predict=predict)


def big_univLogReg(G, y01_train, ind_train=None, ind_col=None, covar_train=None, tol=1e-8, maxiter=20, verbose=True):
    """bigstatsr::big_univLogReg: per variant, the maximum-likelihood coefficient of x in y01 ~ x + 1 + covar, its standard
    error, z-score and the number of solves (`niter`; -1: not converged after `maxiter`, 0 with NaN: missing value, no
    variance or a singular system).  `verbose` (not an argument of bigstatsr's): False silences the one-line message
    that counts the variants whose fit did not converge."""
    ir, image = _train(G, ind_train, ind_col)
    n = ir.size
    y = _y(y01_train, n, "y01.train")
    if not np.all((y == 0) | (y == 1)):
        raise BsnError("'y01.train' should be composed of 0s and 1s.")
    cov = _covar(covar_train, n)
    if int(maxiter) < 1:
        raise BsnError("'maxiter' must be at least 1.")
    im, ir, ic = image()
    q = cov.shape[1]
    estim, se, niter = np.empty(ic.size), np.empty(ic.size), np.empty(ic.size, dtype=np.int32)
    check(_lib.load().bsn_univ_logreg(im.handle, ptr(ir, i64p), n, ptr(ic, i64p), ic.size, ptr(y, f64p),
                                      cov.ctypes.data_as(f64p) if q else None, q, float(tol), int(maxiter),
                                      ptr(estim, f64p), ptr(se, f64p), niter.ctypes.data_as(C.POINTER(C.c_int32))))
    nb = int((niter < 0).sum())
    if nb and verbose:
        print("For %d columns, IRLS didn't converge; `niter` is -1 there and the last iterate is returned "
              "(no `glm` refit)." % nb)
    score = estim / se

    def predict(log10=True):
        from scipy.stats import norm
        lp = (np.log(2.0) + norm.logsf(np.abs(score))) / np.log(10)
        return lp if log10 else 10.0 ** lp
    return dict(estim=estim, std_err=se, score=score, niter=niter, predict=predict)
