"""big_spLinReg / big_spLogReg — host mirror of bigstatsr's penalised regressions (elastic-net paths on individual-level
data with cross-model selection and averaging, CMSA; external to the reference tree like big_randomSVD and
big_univLogReg; vignettes/demo.Rmd:99 and R/SCT.R:278-290 call them).  Indices are 0-based.

What is pinned is the statement of DESIGN.md 3.5i, kept in bigsnpr_amd/csrc/plr_step.hpp, from which both the kernels
(bigsnpr_amd/csrc/plr.hip) and the CPU statement (tests/native/plr_ref.cpp) compile.  bigstatsr's own source is not part
of the reference tree, so parity with its numbers is UNPINNED (as for pca_OADP_proj2): the statement follows its
documented algorithm (biglasso's coordinate descent, early stopping on the validation fold, the four messages) but
scans every column at every lambda instead of screening with the strong rule, standardises with the training rows of
each fold, and counts l = 0 (the unpenalised start) as the first model of a path.

One chain = one (alpha, fold); all chains of a call live on the device together: bsn_bed_sp_reg for a 2-bit or byte
image, bsn_dense_sp_reg for a dense host matrix or a MultiPRS."""
import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._lib import BsnError, PlrOptions, check, f64p, i32p, i64p, ptr

MESSAGES = ("", "No more improvement", "Too many variables", "Model saturated", "Complete path")
_NA_MSG = ("You can't have missing values in 'X'.\nImpute them first (snp_fastImputeSimple) or leave their columns out of "
           "'ind.col'.")


def _is_image(X):
    from .bed import bed
    from .ld import FBM_code256
    return isinstance(X, (bed, FBM_code256))


def _dense(X):
    """a dense host matrix (or a MultiPRS) as a float32 / float64 array"""
    A = np.asarray(getattr(X, "scores", X))
    if A.ndim != 2:
        raise BsnError("'X' must be a matrix.")
    if A.dtype not in (np.float32, np.float64):
        A = A.astype(np.float64)
    return A


def draw_sets(n, K, seed=None):
    """fold ids 0 .. K - 1 as bigstatsr draws them, sample(rep_len(1:K, n)), with numpy's generator"""
    return np.random.default_rng(seed).permutation(np.arange(n) % K).astype(np.int32)


def _sigmoid(s):
    return 1.0 / (1.0 + np.exp(-s))


class BigSpReg(list):
    """list over alphas of lists over folds of dicts (intercept, beta, iter, lambda, alpha, loss, loss_val, nb_active,
    message, ind_col, ind_sets, best); `.family` is "gaussian" or "binomial", `.alphas` the alphas, `.ind_col` the
    columns of X the model was trained on and `.n_covar` the number of covariates behind them in `beta`."""
    family = None
    alphas = None
    ind_col = None
    n_covar = 0

    def summary(self, best_only=False):
        """one row (dict) per alpha: validation_loss (mean over the folds, each at its best lambda), intercept and beta
        averaged over the folds, nb_var (non-zero averaged coefficients), message (per fold), all_conv"""
        rows = []
        for a, mods in zip(self.alphas, self):
            beta = np.mean([mo["beta"] for mo in mods], axis=0)
            msgs = [mo["message"] for mo in mods]
            rows.append(dict(alpha=float(a), validation_loss=float(np.mean([mo["loss_val"][mo["best"]] for mo in mods])),
                             intercept=float(np.mean([mo["intercept"] for mo in mods])), beta=beta,
                             nb_var=int(np.count_nonzero(beta)), message=msgs,
                             all_conv=all(m == "No more improvement" for m in msgs)))
        if best_only:
            return [min(rows, key=lambda r: r["validation_loss"])]
        return rows

    def predict(self, X, ind_row=None, ind_col=None, covar_row=None, proba=True):
        """the best alpha's averaged model on X[ind_row, ind_col] (ind_col defaults to the training columns); `proba`
        applies the logistic function for big_spLogReg models only"""
        best = self.summary(best_only=True)[0]
        ic = self.ind_col if ind_col is None else np.asarray(ind_col, dtype=np.int64)
        m = ic.size
        beta = best["beta"]
        if beta.size != m + self.n_covar:
            raise BsnError("Incompatibility between dimensions.\n'ind.col' and the model's coefficients should have the same length.")
        if _is_image(X):
            from .bed import bed, bed_prodVec
            from .ld import big_prodVec
            s = np.asarray((bed_prodVec if isinstance(X, bed) else big_prodVec)(X, beta[:m], ind_row, ic))
        else:
            A = _dense(X)
            rows = slice(None) if ind_row is None else np.asarray(ind_row, dtype=np.int64)
            s = A[rows][:, ic].astype(np.float64) @ beta[:m]
        s = best["intercept"] + s
        if self.n_covar:
            if covar_row is None:
                raise BsnError("The model was trained with covariates: 'covar.row' is needed.")
            cov = np.asarray(covar_row, dtype=np.float64).reshape(s.size, -1)
            if cov.shape[1] != self.n_covar:
                raise BsnError("Incompatibility between dimensions.\n'covar.row' should have %d columns." % self.n_covar)
            s = s + cov @ beta[m:]
        elif covar_row is not None and np.asarray(covar_row).size:
            raise BsnError("The model was trained without covariates: 'covar.row' must be NULL.")
        return _sigmoid(s) if (proba and self.family == "binomial") else s


def _sp_reg(family, X, y, ind_train, ind_col, covar_train, pf_X, pf_covar, alphas, K, ind_sets, nlambda, lambda_min_ratio,
            nlam_min, n_abort, dfmax, eps, max_iter, warn, seed, kw):
    what = "big_spLogReg" if family else "big_spLinReg"
    yname = "y01.train" if family else "y.train"
    for k in kw:
        if k not in ("base_train", "power_scale", "power_adaptive"):
            raise TypeError("%s() got an unexpected keyword argument '%s'" % (what, k))
    if kw.get("base_train") is not None:
        raise BsnError("%s: 'base.train' is not built." % what)
    if kw.get("power_scale", 1) != 1 or kw.get("power_adaptive", 0) != 0:
        raise BsnError("%s: 'power_scale' != 1 and 'power_adaptive' != 0 are not built." % what)
    image = _is_image(X)
    A = None if image else _dense(X)
    nrow, ncol = (X.nrow, X.ncol) if image else A.shape
    ir = np.arange(nrow, dtype=np.int64) if ind_train is None else np.ascontiguousarray(ind_train, dtype=np.int64).ravel()
    ic = np.arange(ncol, dtype=np.int64) if ind_col is None else np.ascontiguousarray(ind_col, dtype=np.int64).ravel()
    n, m = ir.size, ic.size
    if n == 0 or m == 0:
        raise BsnError("'ind.train' and 'ind.col' can't be empty.")
    if ir.min() < 0 or ir.max() >= nrow or ic.min() < 0 or ic.max() >= ncol:
        raise BsnError("Subscript out of bounds ('ind.train' or 'ind.col').")
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    if y.size != n:
        raise BsnError("Incompatibility between dimensions.\n'%s' and 'ind.train' should have the same length." % yname)
    if not np.all(np.isfinite(y)):
        raise BsnError("You can't have missing values in '%s'." % yname)
    if family and not np.all((y == 0) | (y == 1)):
        raise BsnError("'y01.train' should be composed of 0s and 1s.")
    if covar_train is None:
        cov = np.empty((n, 0), order="F")
    else:
        cov = np.asarray(covar_train, dtype=np.float64)
        cov = np.asfortranarray(cov[:, None] if cov.ndim == 1 else cov)
        if cov.ndim != 2 or cov.shape[0] != n:
            raise BsnError("Incompatibility between dimensions.\n'covar.train' and 'ind.train' should have the same length.")
        if not np.all(np.isfinite(cov)):
            raise BsnError("You can't have missing values in 'covar.train'.")
    q = cov.shape[1]
    pf = np.r_[np.ones(m) if pf_X is None else np.asarray(pf_X, dtype=np.float64).ravel(),
               np.zeros(q) if pf_covar is None else np.asarray(pf_covar, dtype=np.float64).ravel()]
    if pf.size != m + q:
        raise BsnError("Incompatibility between dimensions.\n'pf.X' / 'pf.covar' and the columns should have the same length.")
    if not np.all(np.isfinite(pf)) or np.any(pf < 0):
        raise BsnError("Penalty factors must be finite and non-negative.")
    alphas = np.atleast_1d(np.asarray(alphas, dtype=np.float64)).ravel()
    if alphas.size == 0 or not np.all((alphas > 0) & (alphas <= 1)):
        raise BsnError("'alphas' must be in (0, 1].")
    if ind_sets is None:
        if int(K) < 2:
            raise BsnError("'K' must be at least 2.")
        sets = draw_sets(n, int(K), seed)
    else:
        sets = np.ascontiguousarray(ind_sets).ravel()
        if sets.size != n:
            raise BsnError("Incompatibility between dimensions.\n'ind.sets' and 'ind.train' should have the same length.")
        if not np.all(sets == np.floor(sets)) or sets.min() < 0:
            raise BsnError("'ind.sets' must hold fold ids 0 .. K - 1.")
        sets = sets.astype(np.int32)
        K = int(sets.max()) + 1
        if K < 2:
            raise BsnError("'K' must be at least 2.")
    K = int(K)
    cnt = np.bincount(sets, minlength=K)
    if np.any(cnt == 0) or np.any(cnt == n):
        raise BsnError("Every fold of 'ind.sets' needs at least one row, and so does its training set.")
    if family:
        for k in range(K):
            yt = y[sets != k]
            if yt.min() == yt.max():
                raise BsnError("'y01.train' has a single class among the training rows of fold %d." % k)
    if lambda_min_ratio is None:
        lambda_min_ratio = 1e-4 if n > m else 1e-3
    if int(nlambda) < 2 or int(max_iter) < 1 or int(n_abort) < 1 or int(dfmax) < 1 or int(nlam_min) < 0:
        raise BsnError("'nlambda' >= 2, 'max.iter' >= 1, 'n.abort' >= 1, 'dfmax' >= 1 and 'nlam.min' >= 0 are required.")
    if not (eps > 0) or not (0 < lambda_min_ratio <= 1):
        raise BsnError("'eps' > 0 and 0 < 'lambda.min.ratio' <= 1 are required.")
    if not image and not np.all(np.isfinite(A[np.ix_(ir, ic)] if (ind_train is not None or ind_col is not None) else A)):
        raise BsnError(_NA_MSG)
    opt = PlrOptions(int(family), int(nlambda), int(nlam_min), int(n_abort), int(min(dfmax, 2 ** 31 - 1)), int(max_iter),
                     float(eps), float(lambda_min_ratio))
    NL, Cn, p = int(nlambda), K * alphas.size, m + q
    intercept, beta = np.empty(Cn), np.empty((p, Cn), order="F")
    lam, loss, lossv = (np.empty((NL, Cn), order="F") for _ in range(3))
    it, nb = (np.empty((NL, Cn), dtype=np.int32, order="F") for _ in range(2))
    n_done, best, status = (np.empty(Cn, dtype=np.int32) for _ in range(3))
    tail = [ptr(y, f64p), cov.ctypes.data_as(f64p) if q else None, q, ptr(pf, f64p), ptr(sets, i32p), K, ptr(alphas, f64p),
            alphas.size, C.byref(opt), ptr(intercept, f64p), ptr(beta, f64p), ptr(lam, f64p), ptr(loss, f64p),
            ptr(lossv, f64p), ptr(it, i32p), ptr(nb, i32p), ptr(n_done, i32p), ptr(best, i32p), ptr(status, i32p)]
    lib = _lib.load()
    if image:
        from .ld import _image
        check(lib.bsn_bed_sp_reg(_image(X).handle, ptr(ir, i64p), n, ptr(ic, i64p), m, *tail))
    else:
        # the selection as one F-ordered block in the matrix's own type (float32 stays float32 on the way in)
        whole = ind_train is None and ind_col is None
        B = np.asfortranarray(A if whole else A[np.ix_(ir, ic)])
        check(lib.bsn_dense_sp_reg(B.ctypes.data_as(C.c_void_p), 4 if B.dtype == np.float32 else 7, n, n, m, *tail))
    out = BigSpReg()
    out.family, out.alphas, out.ind_col, out.n_covar = ("binomial" if family else "gaussian"), alphas, ic, q
    for a in range(alphas.size):
        mods = []
        for k in range(K):
            c, d = a * K + k, int(n_done[a * K + k])
            msg = MESSAGES[int(status[c])]
            mods.append(dict(intercept=float(intercept[c]), beta=beta[:, c].copy(), iter=it[:d, c].copy(),
                             **{"lambda": lam[:d, c].copy()}, alpha=float(alphas[a]), loss=loss[:d, c].copy(),
                             loss_val=lossv[:d, c].copy(), nb_active=nb[:d, c].copy(), message=msg, ind_col=ic,
                             ind_sets=sets, best=int(best[c])))
            if warn and msg != "No more improvement":
                warnings.warn("%s: alpha = %g, fold %d ended with \"%s\" instead of \"No more improvement\"; consider other "
                              "'nlambda', 'dfmax' or 'n.abort'." % (what, alphas[a], k, msg))
        out.append(mods)
    return out


def big_spLinReg(X, y_train, ind_train=None, ind_col=None, covar_train=None, pf_X=None, pf_covar=None, alphas=1, K=10,
                 ind_sets=None, nlambda=200, lambda_min_ratio=None, nlam_min=50, n_abort=10, dfmax=50_000, eps=1e-5,
                 max_iter=1000, warn=True, ncores=1, seed=None, **kw):
    """bigstatsr::big_spLinReg: elastic-net linear regression paths for every (alpha, fold), each stopped on its
    validation fold; returns a BigSpReg.  X: a bed / FBM_code256 (2-bit or CODE_DOSAGE-like byte image), a dense float32 /
    float64 matrix, or a MultiPRS.  `ncores` is accepted and ignored; `seed` draws `ind_sets` when it is not given."""
    return _sp_reg(0, X, y_train, ind_train, ind_col, covar_train, pf_X, pf_covar, alphas, K, ind_sets, nlambda,
                   lambda_min_ratio, nlam_min, n_abort, dfmax, eps, max_iter, warn, seed, kw)


def big_spLogReg(X, y01_train, ind_train=None, ind_col=None, covar_train=None, pf_X=None, pf_covar=None, alphas=1, K=10,
                 ind_sets=None, nlambda=200, lambda_min_ratio=None, nlam_min=50, n_abort=10, dfmax=50_000, eps=1e-5,
                 max_iter=1000, warn=True, ncores=1, seed=None, **kw):
    """bigstatsr::big_spLogReg: the same for a 0 / 1 phenotype (penalised logistic regression)."""
    return _sp_reg(1, X, y01_train, ind_train, ind_col, covar_train, pf_X, pf_covar, alphas, K, ind_sets, nlambda,
                   lambda_min_ratio, nlam_min, n_abort, dfmax, eps, max_iter, warn, seed, kw)
