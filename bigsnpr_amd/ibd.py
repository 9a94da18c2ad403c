"""bed_ibd / bed_ibdQC / indep_pairwise — the method-of-moments IBD table of every pair of samples and the removal of
related samples, host mirror of snp_plinkIBDQC (R/external-software.R of the reference) over bsn_bed_ibd
(bigsnpr_amd/csrc/ibd.hip).

The reference hands this step to two PLINK 1.9 child processes (--indep-pairwise, then --genome).  Here the IBS0 / IBS1 /
IBS2 counts of every pair come from the pair kernel of bed_king, the allele-frequency moments from one counting pass over
the founders, and the estimate runs on the device as csrc/ibd_step.hpp states it: PLINK's default ("bounded") Z0, Z1, Z2,
PI_HAT = Z1 / 2 + Z2 and DST.  No PLINK binary exists here to pin it against: the statement in DESIGN.md 3.5p is the
contract, PLINK itself is not emulated bit for bit.

Not emulated: `extra.options`, the RT / EZ / PHE / PPC / RATIO columns of a .genome file, --genome unbounded / nudge,
PLINK's own window walk of --indep-pairwise (`indep_pairwise` states the rule used instead)."""
import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._lib import check, f64p, i32p, i64p, ptr, u8p, vp
from .bed import sub_bed
from .ld import _ind

IBS_NAMES = ("IBS0", "IBS1", "IBS2")
EST_NAMES = ("Z0", "Z1", "Z2", "PI_HAT", "DST")


def _founders(im, ir, founders_only=True):
    """which positions of `ir` count for the allele frequencies: the founders (both parents "0"); without a .fam file, or
    with founders_only=False, every sample"""
    if not founders_only or not getattr(im, "bedfile", None):
        return np.ones(ir.size, dtype=bool)
    fam = im.fam
    return ((np.asarray(fam["paternal_ID"]).astype(str) == "0") & (np.asarray(fam["maternal_ID"]).astype(str) == "0"))[ir]


def _table(im, ir, ic, freq, min_pi_hat, filt):
    lib = _lib.load()
    h, count = vp(), C.c_int64(0)
    mask = None if freq is None else np.ascontiguousarray(freq, dtype=np.uint8)
    check(lib.bsn_bed_ibd(im.handle, ptr(ir, i64p), ir.size, ptr(ic, i64p), ic.size, ptr(mask, u8p), float(min_pi_hat), int(filt),
                          C.byref(count), C.byref(h)))
    try:
        k = int(count.value)
        i1, i2 = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32)
        ibs, est = np.empty((k, 3), dtype=np.int32), np.empty((k, 5))
        E, n_used = np.empty(5), C.c_int64(0)
        check(lib.bsn_ibd_fetch(h, ptr(i1, i32p), ptr(i2, i32p), ptr(ibs, i32p), ptr(est, f64p), ptr(E, f64p), C.byref(n_used)))
    finally:
        lib.bsn_ibd_free(h)
    res = dict(I1=i1, I2=i2)
    for q, name in enumerate(IBS_NAMES):
        res[name] = np.ascontiguousarray(ibs[:, q])
    for q, name in enumerate(EST_NAMES):
        res[name] = np.ascontiguousarray(est[:, q])
    res["E"], res["n_used"] = E, int(n_used.value)
    return res


def bed_ibd(obj_bed, pi_hat=None, ind_row=None, ind_col=None, founders_only=True):
    """The IBD table of the pairs of samples `ind_row` over the variants `ind_col` (what PLINK 1.9's --genome reports): a
    dict of arrays, one entry per pair, ascending in (I1, I2), plus `E` and `n_used`.

    I1 < I2 are positions in `ind_row` (0-based; any list, repeats included).  Over the variants where both samples are
    called: IBS0 (opposite homozygotes), IBS1 (one heterozygous, the other homozygous), IBS2 (the rest); then Z0, Z1, Z2
    (the method-of-moments estimate, bounded as PLINK does by default), PI_HAT = Z1 / 2 + Z2 and DST = (IBS2 + IBS1 / 2) /
    (IBS0 + IBS1 + IBS2).  A pair without a shared call is NaN in the five doubles.  `E` holds the moments E00, E01, E02,
    E11, E12: means over the `n_used` variants that have more than 3 called alleles and both alleles among the frequency
    samples — the founders (paternal.ID and maternal.ID both "0") among `ind_row`; every sample without a .fam file or with
    founders_only=False.  pi_hat = None returns every pair; a number keeps the pairs with PI_HAT >= pi_hat (--min).
    FID1, IID1, FID2, IID2 are added when the object has a .fam file.  The statement in full: DESIGN.md 3.5p."""
    im, ir, ic = _ind(obj_bed, ind_row, ind_col)
    res = _table(im, ir, ic, _founders(im, ir, founders_only), 0.0 if pi_hat is None else pi_hat, pi_hat is not None)
    if getattr(im, "bedfile", None):
        fam = im.fam
        for name, col, idx in (("FID1", "family_ID", "I1"), ("IID1", "sample_ID", "I1"), ("FID2", "family_ID", "I2"),
                               ("IID2", "sample_ID", "I2")):
            res[name] = fam[col][ir[res[idx]]]
    return res


def prune_walk(pair_i, pair_j, maf):
    """The pruning rule of `indep_pairwise` as a pure function: which of maf.size variants are kept, given the pairs
    (i < j) that are in LD.  Pairs are visited with i ascending, then j ascending; a pair with a removed member is skipped;
    otherwise the variant with the smaller `maf` is removed, j on a tie; once i is removed the walk goes on with the next
    i.  Returns a bool mask."""
    maf = np.asarray(maf, dtype=np.float64)
    pi, pj = np.asarray(pair_i, dtype=np.int64).ravel(), np.asarray(pair_j, dtype=np.int64).ravel()
    if pi.size != pj.size:
        raise ValueError("Incompatibility between dimensions.\n'pair_i' and 'pair_j' should have the same length.")
    if pi.size and (pi.min() < 0 or pj.max() >= maf.size or (pi >= pj).any()):
        raise IndexError("'pair_i' < 'pair_j' should index 'maf'.")
    order = np.lexsort((pj, pi))
    removed = np.zeros(maf.size, dtype=bool)
    for i, j in zip(pi[order].tolist(), pj[order].tolist()):
        if removed[i] or removed[j]:
            continue
        if maf[i] < maf[j]:
            removed[i] = True
        else:
            removed[j] = True
    return ~removed


def _chromosomes(im, ic):
    """runs of `ic` by chromosome, each in the order of `ic`: a list of arrays of positions in `ic`"""
    if not getattr(im, "bedfile", None):
        return [np.arange(ic.size)]
    chrom = np.asarray(im.map["chromosome"])[ic]
    _, first, inv = np.unique(chrom, return_index=True, return_inverse=True)
    return [np.flatnonzero(inv == g) for g in np.argsort(first)]


def indep_pairwise(obj_bed, window=100, thr_r2=0.2, ind_row=None, ind_col=None):
    """LD pruning in the manner of PLINK's --indep-pairwise <window> 1 <thr_r2>: the entries of `ind_col` that are kept.

    Per chromosome (from the .bim file; one chromosome without files), variants are taken in the order of `ind_col`.  A
    pair (i < j) with j - i < window is "in LD" iff it is a non-NaN entry of bed_cor(size = window - 1, thr_r2 = thr_r2)
    over the frequency samples (the founders among `ind_row`, as in `bed_ibd`): the r^2 band is computed on the device.
    The pairs in LD are then walked on the host by `prune_walk`, with the minor allele frequency over the same samples.
    PLINK's own window walk (window by window, recomputing after every shift) is NOT emulated."""
    from .bed import bed_counts
    from .ld import bed_cor
    window = int(window)
    if window < 2:
        raise ValueError("'window' should be at least 2 variants.")
    if not 0 <= thr_r2 <= 1:
        raise ValueError("'thr_r2' should be in range [0, 1].")
    im, ir, ic = _ind(obj_bed, ind_row, ind_col)
    rows = ir[_founders(im, ir)]
    if rows.size == 0:
        raise ValueError("indep_pairwise: no founder among 'ind_row'.")
    keep = np.ones(ic.size, dtype=bool)
    for where in _chromosomes(im, ic):
        cols = ic[where]
        if cols.size < 2:
            continue
        c = bed_counts(im, rows, cols).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            p = (c[1] + 2 * c[2]) / (2 * (c[0] + c[1] + c[2]))
        maf = np.minimum(p, 1 - p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (monomorphic variants give NaN entries: they are in LD with nothing)
            cor = bed_cor(im, rows, cols, size=window - 1, thr_r2=thr_r2, fill_diag=False)
        pj = np.repeat(np.arange(cols.size), np.diff(cor.p))
        pi = np.asarray(cor.i, dtype=np.int64)
        ok = ~np.isnan(cor.x) & (pi < pj)
        keep[where] = prune_walk(pi[ok], pj[ok], maf)
    return ic[keep]


def bed_ibdQC(obj_bed, bedfile_out=None, pi_hat=0.08, pruning_args=(100, 0.2), do_blind_QC=True, autosome_only=True, ind_row=None):
    """snp_plinkIBDQC without PLINK; the arguments and their defaults are the reference's.

    1. autosome_only drops the variants outside chromosomes 1 .. 22 (`qc.autosomes`), as --genome ignores them.
    2. Unless pruning_args is None, the variants are pruned by indep_pairwise(window, thr_r2) = pruning_args.
    3. The table of the pairs with PI_HAT >= pi_hat is computed (`bed_ibd`).
    do_blind_QC=False returns that table.  do_blind_QC=True removes the FIRST sample (FID1, IID1) of every reported pair,
    exactly as the reference passes its .genome table to snp_plinkRmSamples: the file is written by bed_plinkRmSamples
    to `bedfile_out` (default "<in>_norel.bed"), which refuses to overwrite, and its path is returned; when no pair is
    reported, a message says so and the path of the input is returned.  `extra.options` has no counterpart."""
    from .qc import _check_out, autosomes, bed_plinkRmSamples
    im, ir, ic = _ind(obj_bed, ind_row, None)
    has_files = bool(getattr(im, "bedfile", None))
    if do_blind_QC:
        if not has_files:
            raise ValueError("bed_ibdQC(do_blind_QC=True) needs a 'bed' object attached to a file (.bim and .fam are copied).")
        bedfile_out = _check_out(sub_bed(im.bedfile) + "_norel.bed" if bedfile_out is None else bedfile_out)
    if autosome_only:
        if not has_files:
            raise ValueError("bed_ibdQC(autosome_only=True) needs a 'bed' object attached to a file (the .bim is read).")
        ic = ic[autosomes(im.map["chromosome"])[ic]]
        if ic.size == 0:
            raise ValueError("bed_ibdQC: no autosomal variant is selected.")
    if pruning_args is not None:
        window, thr_r2 = pruning_args
        ic = indep_pairwise(im, window, thr_r2, ind_row=ir, ind_col=ic)
    table = bed_ibd(im, pi_hat, ir, ic)
    if not do_blind_QC:
        return table
    if table["PI_HAT"].size == 0:
        print("No pair of samples has PI_HAT > %s." % pi_hat)
        return im.bedfile
    return bed_plinkRmSamples(im, bedfile_out, dict(FID=table["FID1"], IID=table["IID1"]), "FID", "IID")


def ibd_last_ms():
    """device ms of the last bed_ibd / bed_ibdQC of this process: the operand, the per-sample totals of the two-product path
    (0 on the general path), the pair kernel, the compaction (as king_last_ms), then the counting pass of the frequency
    samples and the moment kernels (bsn_ibd_last_ms)"""
    ms = (C.c_double * 6)()
    check(_lib.load().bsn_ibd_last_ms(ms))
    return [float(x) for x in ms]
