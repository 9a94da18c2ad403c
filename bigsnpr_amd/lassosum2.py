"""lassosum2 on the device — host mirror of R/lassosum2.R over bigsparser's SFBM.

as_SFBM(corr) puts a sparse LD matrix in HBM once (bsn_sfbm_from_csc); snp_lassosum2 then runs the whole
(lambda, delta) grid over it in one library call (bsn_lassosum2, src/lassosum2.cpp:8-70 for every grid point).  The
results equal the reference's sequential loop bit for bit.  Indices are 0-based."""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import as_f64, check, f64p, i32p, i64p, ptr, vp
from .bed import ERROR_DIM
from .sct import seq_log


class SFBM:
    """A sparse symmetric LD matrix held in HBM as full columns (bigsparser::SFBM).  Reused across calls; free it with
    close() or a `with` block (a finalizer frees it otherwise)."""

    def __init__(self, p, i, x, m2, upper):
        p = np.ascontiguousarray(p, dtype=np.int64)
        i = np.ascontiguousarray(i, dtype=np.int32)
        x = np.ascontiguousarray(x, dtype=np.float64)
        if p.size != m2 + 1:
            raise ValueError("'corr@p' should have ncol(corr) + 1 elements.")
        if i.size != x.size or (p.size and p[-1] != i.size):
            raise ValueError("'corr@i' and 'corr@x' should have corr@p[ncol + 1] elements.")
        h = vp()
        L = _lib.load()
        check(L.bsn_sfbm_from_csc(ptr(p, i64p), ptr(i, i32p), ptr(x, f64p), int(m2), int(bool(upper)), C.byref(h)))
        self.handle = h
        self._fin = weakref.finalize(self, L.bsn_sfbm_free, h)
        info = [C.c_int64(0) for _ in range(3)]
        check(L.bsn_sfbm_ncol(h, *[C.byref(v) for v in info]))
        self.ncol, self.nnz, self.bandwidth = (v.value for v in info)
        self.shape = (self.ncol, self.ncol)
        # crossprod(tril(corr)@x): what snp_ldsplit clamps max_cost with, taken while the entries are on the host
        from .ldsplit import lower_sumsq
        self.sumsq_lower = lower_sumsq(p, i, x, m2, upper)

    def close(self):
        self._fin()
        self.handle = None

    def last_ms(self):
        """device milliseconds (host copies excluded) of the last sp_prodVec / ld_scores_sfbm / sp_solve_sym on this matrix"""
        ms = C.c_double(0.0)
        check(_lib.load().bsn_sfbm_last_ms(self.handle, C.byref(ms)))
        return ms.value

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def as_SFBM(corr, upper=None):
    """bigsparser::as_SFBM: a CorResult of snp_cor / bed_cor (upper triangle with the diagonal), or a square scipy
    sparse matrix — full columns, or a symmetric matrix stored as its upper triangle (taken as such when nothing is
    stored below the diagonal, or when upper=True).  An SFBM is returned as it is."""
    if isinstance(corr, SFBM):
        return corr
    from .ld import CorResult
    if isinstance(corr, CorResult):
        m2 = corr.Dim[1]
        return SFBM(corr.p, corr.i, corr.x, m2, corr.uplo == "U" if upper is None else upper)
    try:
        from scipy import sparse
    except ImportError:  # pragma: no cover
        sparse = None
    if sparse is None or not sparse.issparse(corr):
        raise TypeError("'corr' should be a CorResult, a scipy sparse matrix or an SFBM.")
    if corr.shape[0] != corr.shape[1]:
        raise ValueError("'corr' should be a square matrix.")
    A = sparse.csc_matrix(corr, dtype=np.float64)
    if not A.has_canonical_format:
        A = A.copy()
        A.sum_duplicates()
    if upper is None:
        upper = sparse.tril(A, k=-1).nnz == 0
    return SFBM(A.indptr, A.indices, A.data, A.shape[1], upper)


class LassosumGrid(np.ndarray):
    """beta_grid (m x number of grid points); `.grid_param` holds the columns lambda, delta, num_iter, time and
    sparsity of attr(beta_grid, "grid_param").  `time` is each grid point's run time in seconds on the device clock
    (all grid points of a call run at the same time; the reference times each with system.time)."""
    grid_param = None

    def __array_finalize__(self, obj):
        if obj is not None:
            self.grid_param = getattr(obj, "grid_param", None)


def _col(df, name):
    try:
        has = name in df
    except TypeError:
        has = False
    if not has:
        raise ValueError("'df_beta' should have element '%s'." % name)
    return as_f64(np.ravel(np.asarray(df[name], dtype=np.float64)))


def lassosum2_grid(lambda0, delta, nlambda, lambda_min_ratio):
    """R/lassosum2.R:55-57: seq_log(lambda0, lambda.min.ratio * lambda0, nlambda + 1)[-1], expand.grid order (lambda
    varies fastest)"""
    seq_lam = seq_log(lambda0, lambda_min_ratio * lambda0, nlambda + 1)[1:]
    delta = np.atleast_1d(np.asarray(delta, dtype=np.float64))
    return np.tile(seq_lam, delta.size), np.repeat(delta, seq_lam.size)


def lassosum2_inputs(beta, beta_se, n_eff, delta, nlambda, lambda_min_ratio):
    """R/lassosum2.R:49-57: scale, beta_hat, pf and the grid (lambda, delta) in expand.grid order"""
    N = n_eff
    scale = np.sqrt(N * beta_se ** 2 + beta ** 2)
    beta_hat = as_f64(beta / scale)
    pf = as_f64(np.sqrt(np.max(N) / N))
    lambda0 = np.max(np.abs(beta_hat / pf))
    lam, dlt = lassosum2_grid(lambda0, delta, nlambda, lambda_min_ratio)
    return scale, beta_hat, pf, as_f64(lam), as_f64(dlt)


def snp_lassosum2(corr, df_beta, delta=(0.001, 0.01, 0.1, 1), nlambda=30, lambda_min_ratio=0.01, dfmax=200e3,
                  maxiter=1000, tol=1e-5, ind_corr=None, ncores=1):
    """R/lassosum2.R:25-81.  corr: an SFBM or anything as_SFBM takes (converted for this call only); df_beta: a
    mapping or DataFrame with beta, beta_se, n_eff.  Returns a LassosumGrid (m x G, float64; NaN columns where the
    reference returns NA)."""
    # the reference's checks, in its order, before any device work
    beta, beta_se, n_eff = (_col(df_beta, n) for n in ("beta", "beta_se", "n_eff"))
    m_corr = _ncol(corr)
    ind = np.arange(m_corr, dtype=np.int64) if ind_corr is None else np.ascontiguousarray(np.ravel(ind_corr), dtype=np.int64)
    if ind.size != beta.size:
        raise ValueError(ERROR_DIM + "\nArguments should have the same length.")
    if not np.all((ind >= 0) & (ind < m_corr)):
        raise ValueError("all(ind.corr %in% cols_along(corr)) is not TRUE")
    if not np.all(beta_se > 0):
        raise ValueError("'df_beta$beta_se' should have only positive values.")
    delta = np.atleast_1d(np.asarray(delta, dtype=np.float64))
    if not np.all(delta > 0):
        raise ValueError("'delta' should have only positive values.")
    if not (int(ncores) == ncores and ncores >= 1):
        raise ValueError("'ncores' should be an integer >= 1.")
    if not (beta.size == beta_se.size == n_eff.size):
        raise ValueError(ERROR_DIM + "\nArguments should have the same length.")

    scale, beta_hat, pf, lam, dlt = lassosum2_inputs(beta, beta_se, n_eff, delta, nlambda, lambda_min_ratio)
    G, m = lam.size, beta_hat.size

    own = not isinstance(corr, SFBM)
    sf = as_SFBM(corr)
    try:
        beta_grid = np.empty((m, G), dtype=np.float64, order="F")
        num_iter = np.zeros(G, dtype=np.int32)
        secs = np.zeros(G)
        sub = None if (ind_corr is None and m == sf.ncol) else ind
        check(_lib.load().bsn_lassosum2(sf.handle, ptr(beta_hat, f64p), m, ptr(pf, f64p), ptr(lam, f64p),
                                        ptr(dlt, f64p), G, ptr(sub, i64p), float(dfmax), int(maxiter), float(tol),
                                        beta_grid.ctypes.data_as(f64p), num_iter.ctypes.data_as(i32p),
                                        secs.ctypes.data_as(f64p)))
    finally:
        if own:
            sf.close()
    out = (beta_grid * scale[:, None]).view(LassosumGrid)
    out.grid_param = {"lambda": lam, "delta": dlt, "num_iter": num_iter.astype(np.int64), "time": secs,
                      "sparsity": _col_means_zero(beta_grid)}
    return out


def _ncol(corr):
    if isinstance(corr, SFBM):
        return corr.ncol
    shape = getattr(corr, "Dim", None) or getattr(corr, "shape", None)
    if shape is None:
        raise TypeError("'corr' should be a CorResult, a scipy sparse matrix or an SFBM.")
    return int(shape[1])


def _col_means_zero(B):
    """colMeans(beta_grid == 0): NA (NaN here) for a column of NA"""
    sp = np.mean(B == 0, axis=0) if B.shape[0] else np.full(B.shape[1], np.nan)
    sp[np.isnan(B).any(axis=0)] = np.nan
    return sp
