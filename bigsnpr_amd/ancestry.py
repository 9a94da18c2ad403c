"""snp_ancestry_summary / bed_ancestry — ancestry proportions from allele frequencies (Privé 2022), host mirror of
R/ancestry-summary.R:31-74 over bsn_ancestry_moments / bsn_ancestry_summary / bsn_bed_ancestry (csrc/ancestry.hip, the
rule in csrc/qp_step.hpp).

The reference solves ONE frequency vector per call; the same method is run per individual with freq = genotype / 2
("For individual genotypes, `min_cor` should be larger than 0.6"), in R a loop of quadprog::solve.QP calls.  Here a call
takes B frequency columns, or every selected sample of a resident genotype image (bed_ancestry), one quadratic program per
group of lanes on the device:

    X = P'X0 (L x K),  y = (P'f) o correction,  Dmat = nearPD(X'X),  dvec = X'y
    minimise 1/2 w'Dmat w - dvec'w   subject to   w >= 0  and  sum w = 1 (sum_to_one) or sum w <= 1

by the dual active-set method of Goldfarb & Idnani, which quadprog implements too.  Dmat is positive definite, so the
minimiser is unique: the MINIMISER is what the tests pin (against its definition: feasibility and the KKT conditions),
not quadprog's or Matrix's numbers.

PARITY STATUS of this module: **unpinned** against quadprog and Matrix::nearPD — both are external to the reference tree
and neither is at hand.  nearPD is restated below with the defaults the reference uses."""
import warnings

import numpy as np

from . import _lib
from ._lib import check, f64p, i32p, i64p, ptr
from .bed import ERROR_DIM

MAX_K = 60
MAX_L = 64


class AncestryProportions(np.ndarray):
    """The proportions (K, or one row of K per frequency column / sample), rounded to 7 decimals as the reference rounds.
    `.names`: the column names of `info_freq_ref` when it is a DataFrame, else None; `.cor_each`: the correlation of the
    input frequencies with every reference column; `.cor_pred`: with the predicted frequencies; `.steps`: active-set steps
    of each program (-1: a NaN or an infinity in its input, -2: not solved); `.ms`: device milliseconds of the genotype
    pass, the moment pass and the program kernel; `.unrounded`: the proportions as the device returned them (what the
    tests hold against the KKT conditions)."""
    names = cor_each = cor_pred = steps = ms = unrounded = None

    def __array_finalize__(self, obj):
        if obj is not None:
            for a in ("names", "cor_each", "cor_pred", "steps", "ms", "unrounded"):
                setattr(self, a, getattr(obj, a, None))


def nearPD(x, eig_tol=1e-6, conv_tol=1e-7, posd_tol=1e-8, maxit=100):
    """Matrix::nearPD(x, base.matrix = TRUE) with its defaults (Higham 2002 with Dykstra's correction, infinity norm):
    (matrix, converged).  Restated, not ported: Matrix is external to the reference tree."""
    x = np.array(x, dtype=np.float64)
    n = x.shape[0]
    if x.ndim != 2 or x.shape[1] != n:
        raise ValueError("nearPD: 'x' should be a square matrix.")
    x = (x + x.T) / 2.0
    norm_inf = lambda a: np.abs(a).sum(axis=1).max()   # noqa: E731
    D_S = np.zeros_like(x)
    X = x
    converged = False
    for _ in range(maxit):
        Y = X
        R = Y - D_S
        d, Q = np.linalg.eigh(R)
        d, Q = d[::-1], Q[:, ::-1]
        p = d > eig_tol * d[0]
        if not p.any():
            raise ValueError("Matrix seems negative semi-definite")
        Qp = Q[:, p]
        X = (Qp * d[p]) @ Qp.T
        D_S = X - R
        conv = norm_inf(Y - X) / norm_inf(Y)
        if conv <= conv_tol:
            converged = True
            break
    d, Q = np.linalg.eigh(X)
    d, Q = d[::-1], Q[:, ::-1]
    Eps = posd_tol * abs(d[0])
    if d[n - 1] < Eps:
        d = np.where(d < Eps, Eps, d)
        o_diag = np.diag(X).copy()
        X = (Q * d) @ Q.T
        D = np.sqrt(np.maximum(Eps, o_diag) / np.diag(X))
        X = D[:, None] * X * D[None, :]
    return (X + X.T) / 2.0, converged


def _names(info_freq_ref):
    cols = getattr(info_freq_ref, "columns", None)
    return None if cols is None else [str(c) for c in cols]


def _assert_nona(a, name):
    if np.isnan(a).any():
        raise ValueError("You can't have missing values in '%s'." % name)


def _tables(info_freq_ref, projection, correction):
    """X0 (M x K), P (M x L), correction (L): checked in the reference's order (freq is checked by the caller first)"""
    X0 = np.asfortranarray(np.asarray(info_freq_ref, dtype=np.float64))
    P = np.asfortranarray(np.asarray(projection, dtype=np.float64))
    if X0.ndim == 1:
        X0 = np.asfortranarray(X0[:, None])
    if P.ndim == 1:
        P = np.asfortranarray(P[:, None])
    _assert_nona(X0, "info_freq_ref")
    _assert_nona(P, "projection")
    return X0, P, np.ascontiguousarray(np.ravel(correction), dtype=np.float64)


def _check_sizes(M, X0, P, corr):
    if X0.shape[0] != M or P.shape[0] != M:
        raise ValueError(ERROR_DIM + "\nArguments should have the same length.")
    if corr.size != P.shape[1]:
        raise ValueError(ERROR_DIM + "\nArguments should have the same length.")
    if not 1 <= X0.shape[1] <= MAX_K:
        raise ValueError("'info_freq_ref' should have between 1 and %d columns." % MAX_K)
    if not 1 <= P.shape[1] <= MAX_L:
        raise ValueError("'projection' should have between 1 and %d columns." % MAX_L)


def _dmat(X):
    Dmat, ok = nearPD(X.T @ X)
    if not ok:
        raise ValueError("Could not find nearest positive definite matrix.")
    return np.asfortranarray(Dmat)


def _wrap(w, names, cor_each, cor_pred, steps, ms):
    out = np.round(w, 7).view(AncestryProportions)
    out.names, out.cor_each, out.cor_pred, out.steps, out.ms = names, cor_each, cor_pred, steps, ms
    out.unrounded = w
    return out


def ancestry_last_ms():
    """device milliseconds of the last ancestry call of this process: [genotype pass, moment pass, program kernel]"""
    ms = np.zeros(3)
    check(_lib.load().bsn_ancestry_last_ms(ptr(ms, f64p)))
    return ms


def qp_simplex(D, d, sum_to_one=True):
    """The primitive (bsn_qp_simplex): minimise 1/2 w'D w - d'w over the simplex (sum w = 1, or sum w <= 1) for every
    column of `d` (K, or K x B).  dict(w: B x K, steps: B, n_failed: programs that reached the step cap)."""
    D = np.asfortranarray(np.asarray(D, dtype=np.float64))
    d = np.asfortranarray(np.asarray(d, dtype=np.float64))
    if d.ndim == 1:
        d = np.asfortranarray(d[:, None])
    if D.ndim != 2 or D.shape[0] != D.shape[1] or d.shape[0] != D.shape[0]:
        raise ValueError(ERROR_DIM)
    K, B = d.shape
    w = np.empty((B, K), order="F")
    steps = np.empty(B, dtype=np.int32)
    nf = np.zeros(1, dtype=np.int64)
    check(_lib.load().bsn_qp_simplex(ptr(D, f64p), K, ptr(d, f64p), B, int(bool(sum_to_one)), ptr(w, f64p), ptr(steps, i32p),
                                     ptr(nf, i64p)))
    return dict(w=w, steps=steps, n_failed=int(nf[0]))


def ancestry_moments(P, X0, F=None, ld=None):
    """The moment pass (bsn_ancestry_moments) on host matrices: dict(PtX0, PtF, G0 = X0'X0, X0tF, csX0, csF, sqF).
    ld: hand the matrices over as the top rows of matrices of `ld` rows (NaN below)."""
    P = np.asfortranarray(np.asarray(P, dtype=np.float64))
    X0 = np.asfortranarray(np.asarray(X0, dtype=np.float64))
    M, L = P.shape
    K = X0.shape[1]
    F = np.zeros((M, 0), order="F") if F is None else np.asfortranarray(np.asarray(F, dtype=np.float64))
    if F.ndim == 1:
        F = np.asfortranarray(F[:, None])
    B = F.shape[1]
    if X0.shape[0] != M or F.shape[0] != M:
        raise ValueError(ERROR_DIM)

    def pad(a):
        if ld is None:
            return a
        out = np.full((ld, a.shape[1]), np.nan, order="F")
        out[:M] = a
        return out
    P, X0, F = pad(P), pad(X0), pad(F)
    lead = M if ld is None else ld
    out = dict(PtX0=np.zeros((L, K), order="F"), PtF=np.zeros((L, B), order="F"), G0=np.zeros((K, K), order="F"),
               X0tF=np.zeros((K, B), order="F"), csX0=np.zeros(K), csF=np.zeros(B), sqF=np.zeros(B))
    check(_lib.load().bsn_ancestry_moments(ptr(P, f64p), lead, ptr(X0, f64p), lead, ptr(F, f64p) if B else None, lead, M, L, K, B, 0,
                                           *[ptr(out[k], f64p) for k in ("PtX0", "PtF", "G0", "X0tF", "csX0", "csF", "sqF")]))
    return out


def _cor_host(X0, F):
    """cor(X0, F): K x B, on the host (the reference's check comes before any other work)"""
    Xc = X0 - X0.mean(axis=0)
    Fc = F - F.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (Xc.T @ Fc) / np.sqrt(np.outer((Xc * Xc).sum(axis=0), (Fc * Fc).sum(axis=0)))


def snp_ancestry_summary(freq, info_freq_ref, projection, correction, min_cor=0.4, sum_to_one=True):
    """R/ancestry-summary.R:31-74.  `freq`: M frequencies, or M x B (one problem per column).  Match the variants with
    snp_match first and reverse the frequencies accordingly, as for the reference.

    Returns AncestryProportions: K values for a vector (`cor_pred < min_cor` raises the reference's error, `< 0.99`
    warns), B x K for a matrix (a column whose frequencies seem reversed, or whose `cor_pred` is below `min_cor`, comes
    back as a NaN row; nothing is raised).  Unpinned against quadprog / Matrix::nearPD (module docstring)."""
    F = np.asarray(getattr(freq, "values", freq), dtype=np.float64)
    one = F.ndim == 1
    F = np.asfortranarray(F[:, None] if one else F)
    if F.ndim != 2:
        raise ValueError("'freq' should be a vector or a matrix.")
    _assert_nona(F, "freq")
    X0, P, corr = _tables(info_freq_ref, projection, correction)
    M, B = F.shape
    _check_sizes(M, X0, P, corr)
    K, L = X0.shape[1], P.shape[1]
    reversed_ = np.nanmean(_cor_host(X0, F), axis=0) < -0.2 if M > 1 else np.zeros(B, dtype=bool)
    if one and reversed_[0]:
        raise ValueError("Frequencies seem all reversed; switch reference allele?")

    lib = _lib.load()
    d_P, d_X0, d_F = (_lib.DeviceArray.from_numpy(a) for a in (P, X0, F))
    try:
        X = np.zeros((L, K), order="F")
        G0, c0 = np.zeros((K, K), order="F"), np.zeros(K)
        check(lib.bsn_ancestry_moments(d_P.ptr, M, d_X0.ptr, M, None, M, M, L, K, 0, 1, ptr(X, f64p), None, ptr(G0, f64p), None,
                                       ptr(c0, f64p), None, None))
        ms_moments = ancestry_last_ms()[1]
        Dmat = _dmat(X)
        w, ce = np.empty((B, K), order="F"), np.empty((B, K), order="F")
        cp, steps = np.empty(B), np.empty(B, dtype=np.int32)
        check(lib.bsn_ancestry_summary(d_F.ptr, M, B, d_X0.ptr, M, d_P.ptr, M, ptr(corr, f64p), M, L, K, ptr(Dmat, f64p),
                                       int(bool(sum_to_one)), 1, ptr(w, f64p), ptr(ce, f64p), ptr(cp, f64p), ptr(steps, i32p)))
    finally:
        for d in (d_P, d_X0, d_F):
            d.free()
    ms = ancestry_last_ms()
    ms[1] += ms_moments
    return _finish_summary(one, reversed_, w, ce, cp, steps, _names(info_freq_ref), ms, min_cor)


def _finish_summary(one, reversed_, w, ce, cp, steps, names, ms, min_cor):
    """what follows the device calls (R/ancestry-summary.R:63-73): the error and the warning of a vector, the NaN rows of
    a matrix"""
    if one:
        if not cp[0] >= min_cor:
            raise ValueError("Correlation between frequencies is too low: %.3f; check matching between variants." % cp[0])
        if cp[0] < 0.99:
            warnings.warn("The solution does not perfectly match the frequencies.")
        return _wrap(w[0], names, ce[0], float(cp[0]), int(steps[0]), ms)
    w[reversed_ | ~(cp >= min_cor)] = np.nan
    return _wrap(w, names, ce, cp, steps, ms)


def bed_ancestry(obj, info_freq_ref, projection, correction, ind_row=None, ind_col=None, min_cor=0.6, sum_to_one=True):
    """snp_ancestry_summary for every selected sample of a resident genotype image, freq = genotype / 2, in one call
    (bsn_bed_ancestry).  `info_freq_ref` and `projection` have one row per selected column; a missing genotype counts as
    the mean reference frequency of its variant, so a sample's row does not depend on which other rows are selected.
    Returns AncestryProportions, n x K, with the attributes per sample; rows whose `cor_pred` is below `min_cor` are NaN.
    An FBM.code256 handle is served where the genotype product serves it (codes that decode to 0 / 1 / 2 / NA); a dosage
    or generic handle is refused with a message.  Matching and allele reversal are the caller's, as in the reference."""
    from .ld import _ind
    obj, ir, ic = _ind(obj, ind_row, ind_col)
    X0, P, corr = _tables(info_freq_ref, projection, correction)
    _check_sizes(ic.size, X0, P, corr)
    K, L = X0.shape[1], P.shape[1]
    n = ir.size
    X = ancestry_moments(P, X0)["PtX0"]
    ms_moments = ancestry_last_ms()[1]
    Dmat = _dmat(X)
    w, ce = np.empty((n, K), order="F"), np.empty((n, K), order="F")
    cp, steps = np.empty(n), np.empty(n, dtype=np.int32)
    check(_lib.load().bsn_bed_ancestry(obj.handle, ptr(ir, i64p), n, ptr(ic, i64p), ic.size, ptr(X0, f64p), ptr(P, f64p),
                                       ptr(corr, f64p), L, K, ptr(Dmat, f64p), ptr(X, f64p), int(bool(sum_to_one)), ptr(w, f64p),
                                       ptr(ce, f64p), ptr(cp, f64p), ptr(steps, i32p)))
    ms = ancestry_last_ms()
    ms[1] += ms_moments
    w[~(cp >= min_cor)] = np.nan
    return _wrap(w, _names(info_freq_ref), ce, cp, steps, ms)
