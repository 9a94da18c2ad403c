"""Per-group genotype counts, snp_fst and snp_MAX3 — host mirror of R/Fst.R and R/MAX3.R over bsn_bed_group_counts,
bsn_fst, bsn_bed_fst and bsn_snp_max3 (bigsnpr_amd/csrc/popstat.hip).

The reference counts one population per call of bed_MAF / big_counts — one pass over the genotype matrix each — and
evaluates the statistics in R.  Here one pass counts up to 32 groups (`bed_counts_by_group`, `bed_MAF_by_group`), and
`bed_fst` / `snp_MAX3` evaluate the statistic on the device from the counts, which never leave it."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f64p, i32p, i64p, ptr
from .ld import _ind


def _labels(group, n, n_groups):
    g = np.asarray(group)
    if g.ndim != 1 or g.size != n:
        raise ValueError("Incompatibility between dimensions.\n'group' and 'ind.row' should have the same length.")
    g = np.clip(g.astype(np.int64), -2, 2 ** 31 - 1)     # (whatever lies outside stays outside; the library names it)
    G = (int(g.max()) + 1 if g.size else 0) if n_groups is None else int(n_groups)
    return np.ascontiguousarray(g, dtype=np.int32), G


def bed_counts_by_group(obj, group, ind_row=None, ind_col=None, n_groups=None):
    """counts of 0, 1, 2, NA of every selected variant among the selected rows of each group, in one pass: an int32 array
    (G, 4, m) whose slice g is what bed_counts(obj, ind_row = the rows labelled g) returns.  group[i] is the label
    0 .. G - 1 of row ind_row[i], or -1 for a row in no group; G = n_groups, or the largest label + 1."""
    im, ir, ic = _ind(obj, ind_row, ind_col)
    g, G = _labels(group, ir.size, n_groups)
    res = np.empty((ic.size, max(G, 0), 4), dtype=np.int32)
    check(_lib.load().bsn_bed_group_counts(im.handle, ptr(ir, i64p), ir.size, ptr(g, i32p), G, ptr(ic, i64p), ic.size,
                                           ptr(res, i32p)))
    return res.transpose(1, 2, 0)     # (a view, like the `res.T` of bed_counts: the library's table is variant-major)


def bed_MAF_by_group(obj, group, ind_row=None, ind_col=None, n_groups=None):
    """a list with, for every group, the dict bed_MAF returns for its rows (R/binom-scaling.R:203-222) — what snp_fst
    takes — from one counting pass"""
    counts = bed_counts_by_group(obj, group, ind_row, ind_col, n_groups).astype(np.int64)
    out = []
    for c in counts:
        ac = c[1] + 2 * c[2]
        nb_nona = c[0] + c[1] + c[2]
        with np.errstate(all="ignore"):
            af = ac / (2.0 * nb_nona)
        out.append(dict(ac=ac, mac=np.minimum(ac, 2 * nb_nona - ac), af=af, maf=np.minimum(af, 1 - af), N=nb_nona))
    return out


def _fst_result(fst, ov, overall):
    return float(ov[0]) if overall else fst


def snp_fst(list_df_af, min_maf=0, overall=False):
    """R/Fst.R:47-85: Weir & Cockerham's Fst from a list of per-population dicts with `af` and `N` (bed_MAF,
    bed_MAF_by_group): per variant (NaN where the variant does not pass `min_maf`), or genome-wide (overall=True)."""
    for df_af in list_df_af:
        for name in ("af", "N"):
            if name not in df_af:
                raise ValueError("'df_af' should have element '%s'." % name)
    r = len(list_df_af)
    if r == 0:
        af = N = np.zeros((0, 1))
    else:
        af = np.ascontiguousarray(np.stack([np.asarray(d["af"], dtype=np.float64) for d in list_df_af]))
        N = np.ascontiguousarray(np.stack([np.asarray(d["N"], dtype=np.float64) for d in list_df_af]))
        if af.ndim != 2 or af.shape != N.shape:
            raise ValueError("Incompatibility between dimensions.")
    m = af.shape[1]
    fst = None if overall else np.empty(m)
    ov = np.empty(3) if overall else None
    check(_lib.load().bsn_fst(ptr(af, f64p), ptr(N, f64p), r, m, float(min_maf), ptr(fst, f64p), ptr(ov, f64p)))
    return _fst_result(fst, ov, overall)


def bed_fst(obj, group, ind_row=None, ind_col=None, min_maf=0, overall=False, n_groups=None):
    """snp_fst(bed_MAF_by_group(obj, group, ...), min_maf, overall) without the frequencies leaving the device: one
    counting pass, the statistic from the device-resident counts, bit-identical to the two-step form."""
    im, ir, ic = _ind(obj, ind_row, ind_col)
    g, G = _labels(group, ir.size, n_groups)
    fst = None if overall else np.empty(ic.size)
    ov = np.empty(3) if overall else None
    check(_lib.load().bsn_bed_fst(im.handle, ptr(ir, i64p), ir.size, ptr(g, i32p), G, ptr(ic, i64p), ic.size, float(min_maf),
                                  ptr(fst, f64p), ptr(ov, f64p)))
    return _fst_result(fst, ov, overall)


def snp_MAX3(Gna, y01_train, ind_train=None, val=(0, 0.5, 1), ind_col=None):
    """R/MAX3.R:81-107: score[j] = max over x in `val` of the squared trend statistic with genotype scores (0, x, 1) between
    the cases (y01_train == 1) and the controls (== 0) among the rows `ind_train`; missing genotypes are left out.
    val = (0, 0.5, 1) is MAX3, (0, 1) MAX2, (0.5,) the Armitage trend test, linspace(0, 1, L) MAXL.  `predict()` gives the
    log10 p-values of a chi-square with one degree of freedom (biased downward for more than one value, like the
    reference's)."""
    im, ir, ic = _ind(Gna, ind_train, ind_col)
    y = np.asarray(y01_train, dtype=np.float64).ravel()
    if y.size != ir.size:
        raise ValueError("Incompatibility between dimensions.\n'ind.train' and 'y01.train' should have the same length.")
    y32 = np.ascontiguousarray(np.where(y == np.floor(y), np.clip(y, -1, 2), 2), dtype=np.int32)
    v = np.ascontiguousarray(np.atleast_1d(val), dtype=np.float64).ravel()
    score = np.empty(ic.size)
    check(_lib.load().bsn_snp_max3(im.handle, ptr(ir, i64p), ir.size, ptr(y32, i32p), ptr(ic, i64p), ic.size, ptr(v, f64p),
                                   v.size, ptr(score, f64p)))

    def predict(log10=True):
        from scipy.stats import chi2
        lp = chi2.logsf(score, 1) / np.log(10)
        return lp if log10 else 10.0 ** lp
    return dict(score=score, predict=predict)


def popstat_last_ms():
    """device ms of the last call above: panel, streaming launches, finalising kernels, statistic (bsn_popstat_last_ms)"""
    ms = (C.c_double * 4)()
    check(_lib.load().bsn_popstat_last_ms(ms))
    return [float(x) for x in ms]
