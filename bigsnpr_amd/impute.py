"""snp_fastImputeSimple — host mirror of R/impute.R:189-203 over bsn_impute_simple (bigsnpr_amd/csrc/impute.hip).

The reference rewrites the FBM's file in place and returns the same file under another decode table; here the source
stays as it is and the result is a NEW FBM_code256 on the device: the 2-bit image of CODE_IMPUTE_PRED for `mode`,
`mean0` and `random`, the int8 grid image of CODE_DOSAGE for `mean2`.  What the reference's file would hold is
available as `.bytes` (return_bytes=True).

What differs from the reference: `random` draws from the library's counter-based generator keyed by `seed`, not from
R's; a variant without any observed call stays missing under `mean0`, `mean2` and `random` (the reference casts a NaN to
a byte there) and is counted in `.n_all_missing`; `Gna` may also be a `bed`."""
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
