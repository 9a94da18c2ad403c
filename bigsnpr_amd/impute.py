"""snp_fastImputeSimple — host mirror of R/impute.R:189-203 over bsn_impute_simple (bigsnpr_amd/csrc/impute.hip).

The reference rewrites the FBM's file in place and returns the same file under another decode table; here the source
stays as it is and the result is a NEW FBM_code256 on the device: the 2-bit image of CODE_IMPUTE_PRED for `mode`,
`mean0` and `random`, the int8 grid image of CODE_DOSAGE for `mean2`.  What the reference's file would hold is
available as `.bytes` (return_bytes=True).

What differs from the reference: `random` draws from the library's counter-based generator keyed by `seed`, not from
R's; a variant without any observed call stays missing under `mean0`, `mean2` and `random` (the reference casts a NaN to
a byte there) and is counted in `.n_all_missing`; `Gna` may also be a `bed`.

snp_fastImpute — host mirror of R/impute.R:29-160 over bsn_fast_impute (bigsnpr_amd/csrc/fastimpute.hip): the predictor
lists from snp_cor per chromosome, then one call that trains an independent boosted-tree model per variant on the device.
Its docstring states what differs from the reference."""
import ctypes as C
import os
import warnings

import numpy as np

from . import _lib
from ._lib import check, u8p, vp
from .bed import bed
from .ld import CODE_012, CODE_DOSAGE, CODE_IMPUTE_PRED, FBM_code256

METHODS = ("mode", "mean0", "mean2", "random")   # R/impute.R:190; their position + 1 is the library's `method`
CODE_ZERO = np.array([0, 1, 2, 0] + [np.nan] * 252)   # R/impute.R:197


def snp_fastImputeSimple(Gna, method="mode", ncores=1, seed=None, return_bytes=False):
    """A new FBM_code256 with every missing genotype of `Gna` (an FBM_code256 with CODE_012, or a `bed`) replaced per
    variant by the most frequent call ("mode"), the mean rounded to 0 ("mean0") or 2 decimal places ("mean2"), or a draw
    from Binomial(2, allele frequency) ("random").  `.seed` is the key of the draws (seed=None: a fresh one),
    `.n_all_missing` the number of variants without any call, `.bytes` (return_bytes=True) the n x m bytes the
    reference's FBM file would hold.  `ncores` is accepted and dropped."""
    if isinstance(Gna, FBM_code256):
        if not np.array_equal(Gna.code256, CODE_012, equal_nan=True):
            raise ValueError("identical(Gna$code256, CODE_012) is not TRUE")
        im = Gna._bed
    elif isinstance(Gna, bed):
        im = Gna
    else:
        raise TypeError("'Gna' is not of class 'FBM.code256' (or 'bed').")
    if method == "zero":
        warnings.warn("Using 'method = \"zero\"' is deprecated. Using $copy() instead..", stacklevel=2)
        num, code = 0, CODE_ZERO
    elif method in METHODS:
        num = METHODS.index(method) + 1
        code = CODE_DOSAGE if method == "mean2" else CODE_IMPUTE_PRED
    else:
        raise ValueError("'method' should be one of %s." % ", ".join('"%s"' % s for s in METHODS))
    seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & (2 ** 64 - 1)
    n, m = im.nrow, im.ncol
    out = np.empty((n, m), dtype=np.uint8, order="F") if return_bytes else None
    h, n_all = vp(), C.c_int64(0)
    check(_lib.load().bsn_impute_simple(im.handle, num, seed, C.byref(h), None if out is None else out.ctypes.data_as(u8p),
                                        C.byref(n_all)))
    res = FBM_code256._from_handle(h, n, m, code)
    res.seed = seed
    res.n_all_missing = int(n_all.value)
    if return_bytes:
        res.bytes = out
    if res.n_all_missing > 0:
        kept = "" if method in ("zero", "mode") else "; they stay missing"
        warnings.warn("%d variants have no observed genotype%s." % (res.n_all_missing, kept), stacklevel=2)
    return res


# ---- snp_fastImpute (R/impute.R:29-160) over bsn_fast_impute (bigsnpr_amd/csrc/fastimpute.hip) -------------------------------
MIN_PREDICTORS = 5   # R/impute.R:70: with fewer correlated variants, the neighbours within `size` are taken instead


def predictor_lists(m, chromosomes, size):
    """The predictor list of every variant as (pred_off int64 [m + 1], pred_idx int32), R/impute.R:69-71.
    `chromosomes`: one (ind_chr, i, p, x) per chromosome — its ascending variant indices and the slots of the upper
    triangle of their sparse correlation matrix (snp_cor with fill_diag=False).  The predictors of a variant are the
    variants of its chromosome whose correlation with it is stored and neither 0 nor NaN (the matrix is symmetric:
    both triangles count); with fewer than 5 of them, the variants of the chromosome whose index lies within +-`size`
    of its own, itself excluded.  Ascending in every list."""
    size = int(size)
    lists = [np.zeros(0, dtype=np.int64)] * m
    for ind_chr, i, p, x in chromosomes:
        ind_chr = np.asarray(ind_chr, dtype=np.int64)
        mc = ind_chr.size
        i, p, x = np.asarray(i, dtype=np.int64), np.asarray(p, dtype=np.int64), np.asarray(x, dtype=np.float64)
        col = np.repeat(np.arange(mc, dtype=np.int64), np.diff(p))
        keep = (x != 0) & ~np.isnan(x) & (i != col)
        r, c = np.concatenate([i[keep], col[keep]]), np.concatenate([col[keep], i[keep]])   # both triangles
        pair = np.unique(c * mc + r)                      # sorted by target, then by predictor
        c, r = pair // mc, pair % mc
        start = np.searchsorted(c, np.arange(mc + 1))
        for k in range(mc):
            got = ind_chr[r[start[k]:start[k + 1]]]
            if got.size < MIN_PREDICTORS:
                snp = ind_chr[k]
                lo, hi = np.searchsorted(ind_chr, snp - size), np.searchsorted(ind_chr, snp + size, side="right")
                got = ind_chr[lo:hi]
                got = got[got != snp]
            lists[int(ind_chr[k])] = got
    off = np.zeros(m + 1, dtype=np.int64)
    off[1:] = np.cumsum([g.size for g in lists])
    idx = np.concatenate(lists + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return off, np.ascontiguousarray(idx)


def snp_fastImpute(Gna, infos_chr, alpha=1e-4, size=200, p_train=0.8, n_cor=None, seed=None, ncores=1, return_bytes=False):
    """A new FBM_code256 (decode table CODE_IMPUTE_PRED) with every missing genotype of `Gna` (an FBM_code256 with
    CODE_012, or a `bed`) replaced by the call of a local boosted-tree model, one model per variant, trained on the
    device.  Per chromosome, snp_cor over a sorted sample of `n_cor` rows (all by default) with `size` and `alpha`
    names the predictors of every variant (predictor_lists); one bsn_fast_impute call then serves all chromosomes.
    `.infos` is what the reference returns: 2 x m, the share of missing calls and the share of wrong calls on the
    validation samples (NaN where there is no model or no validation sample).  `.seed` keys the training split and the
    row sample (seed=None: a fresh one), `.n_all_missing` counts the variants without any observed call (they stay
    missing), `.pred_off` / `.pred_idx` are the predictor lists the call received, `.bytes` (return_bytes=True) the
    n x m bytes the reference's FBM file would hold.  `ncores` is accepted and dropped.

    Deliberate differences from the reference:
    1. Predictors are the SOURCE's codes, and a missing predictor follows the split's default direction.  The reference
       lets a model see the calls imputed for the variants before it, which makes its result depend on their order.
    2. The training split is a Bernoulli(p_train) draw per observed sample from the library's counter-based generator;
       the reference takes exactly floor(p.train * c) samples from R's generator (`seed + i` is not reproduced).
    3. xgboost is not emulated bit for bit.  The tree rule is its exact greedy enumeration with the reference's
       parameters (binary:logistic, max_depth 4, 10 rounds, eta 0.3, lambda 1, gamma 0, min_child_weight 1, base_score
       the clamped training mean), on fp64 gradients quantised to 2^-30 where xgboost uses float32.
    4. The reference's resume file (-infos-impute.rds) is not kept."""
    if isinstance(Gna, FBM_code256):
        if not np.array_equal(Gna.code256, CODE_012, equal_nan=True):
            raise ValueError("identical(Gna$code256, CODE_012) is not TRUE")
        im = Gna._bed
    elif isinstance(Gna, bed):
        im = Gna
    else:
        raise TypeError("'Gna' is not of class 'FBM.code256' (or 'bed').")
    n, m = im.nrow, im.ncol
    infos_chr = np.ravel(np.asarray(infos_chr))
    if infos_chr.size != m:
        raise ValueError("Incompatibility between dimensions.")
    if not 0 < p_train <= 1:
        raise ValueError("'p_train' must lie in (0, 1].")
    if not 0 < alpha <= 1:
        raise ValueError("'alpha' must lie in (0, 1].")
    if int(size) < 1:
        raise ValueError("'size' must be at least 1.")
    n_cor = n if n_cor is None else int(n_cor)
    if not 2 <= n_cor <= n:
        raise ValueError("'n_cor' must lie in [2, %d]." % n)
    seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & (2 ** 64 - 1)
    from .ld import chr_groups, snp_cor
    rng = np.random.default_rng(seed)
    chromosomes = []
    for _, ind_chr in chr_groups(infos_chr):
        rows = np.sort(rng.choice(n, size=n_cor, replace=False)).astype(np.int64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # NaN correlations (a constant variant) name no predictor
            cor = snp_cor(Gna, ind_row=rows, ind_col=ind_chr, size=size, alpha=alpha, fill_diag=False)
        chromosomes.append((ind_chr, cor.i, cor.p, cor.x))
    off, idx = predictor_lists(m, chromosomes, size)
    out = np.empty((n, m), dtype=np.uint8, order="F") if return_bytes else None
    infos = np.empty((2, m), dtype=np.float64)
    h, n_all = vp(), C.c_int64(0)
    check(_lib.load().bsn_fast_impute(im.handle, off.ctypes.data_as(_lib.i64p), idx.ctypes.data_as(_lib.i32p), float(p_train),
                                      seed, C.byref(h), None if out is None else out.ctypes.data_as(u8p),
                                      infos.ctypes.data_as(_lib.f64p), C.byref(n_all)))
    res = FBM_code256._from_handle(h, n, m, CODE_IMPUTE_PRED)
    res.infos, res.seed, res.n_all_missing = infos, seed, int(n_all.value)
    res.pred_off, res.pred_idx = off, idx
    if return_bytes:
        res.bytes = out
    if res.n_all_missing > 0:
        warnings.warn("%d variants have no observed genotype; they stay missing." % res.n_all_missing, stacklevel=2)
    return res
