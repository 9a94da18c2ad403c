"""bed_hwe / bed_plinkQC / bed_plinkRmSamples — the exact Hardy-Weinberg test and the quality-control filters, host mirror
of snp_plinkQC and snp_plinkRmSamples (R/external-software.R:247-343) over bsn_hwe, bsn_bed_hwe and bsn_bed_qc
(bigsnpr_amd/csrc/qc.hip).

The reference hands this step to a PLINK 1.9 child process (--maf --mind --geno --hwe [--autosome] --make-bed).  Here the
counts are taken on the device from the handle's 2-bit image, the exact test of Wigginton, Cutler & Abecasis (2005) runs
there as csrc/hwe_step.hpp states it, and the subset file is written through snp_writeBed.

Which samples count follows PLINK 1.9's documentation of --maf / --hwe; no PLINK binary exists here to pin it against, so
the rules are stated in full (`qc_classes`):
  * a founder has paternal.ID and maternal.ID both "0"; --maf and --hwe count founders only, --mind and --geno everyone;
  * when every `affection` is one of -9, 0, 1, 2 and at least one is 1 (case/control data with controls), --hwe counts the
    founders with affection 1 (the controls) only; otherwise every founder;
  * founders_only=False / hwe_controls_only=False switch either rule off.
The order is PLINK's: samples by --mind first, then all variant filters over the remaining samples at once, so that no
variant filter changes what another one sees.  Not emulated: `extra.options`, `file.type` other than bed, the other
modifiers of --hwe, any special handling of the X chromosome (every variant is tested as diploid)."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import check, f64p, i32p, i64p, ptr, u8p
from .bed import sub_bed
from .ld import _ind

INT32_MAX = 2 ** 31 - 1


def hwe_exact_counts(counts, midp=False):
    """Exact Hardy-Weinberg p-value per variant from a 3 x m table of genotype counts: the homozygotes of one allele, the
    heterozygotes, the homozygotes of the other (what `bed_counts` returns in its first three rows, in either order of the
    alleles).  midp=True is the mid-p variant (half the weight of the observed table and of its ties).  A variant without
    any genotype gives NaN, a monomorphic one 1.  The test sums probability ratios relative to the observed table in
    double precision: a p-value below about 1e-300 may come back as exactly 0."""
    c = np.asarray(counts)
    if c.ndim == 1 and c.size == 3:
        c = c.reshape(3, 1)
    if c.ndim != 2 or c.shape[0] != 3:
        raise ValueError("'counts' should have 3 rows (hom1, het, hom2).")
    c = c.astype(np.int64)
    if c.size and c.max() > INT32_MAX:
        raise ValueError("'counts' holds a value above a 32-bit count.")
    c = np.ascontiguousarray(np.maximum(c, -1).T, dtype=np.int32)     # (a negative count stays negative: the library names it)
    m = c.shape[0]
    p = np.empty(m)
    check(_lib.load().bsn_hwe(ptr(c, i32p), m, int(bool(midp)), ptr(p, f64p)))
    return p


def _hwe_lanes(counts, midp, lanes):
    """(p, device ms) of the test kernel in the form `lanes` (1, 2, or 0 for the default): tests and tools/probe_qc.py"""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.int32).reshape(3, -1).T)
    p, ms = np.empty(c.shape[0]), C.c_double(0.0)
    check(_lib.load().bsn_hwe_lanes(ptr(c, i32p), c.shape[0], int(bool(midp)), int(lanes), ptr(p, f64p), C.byref(ms)))
    return p, float(ms.value)


def bed_hwe(obj_bed, ind_row=None, ind_col=None, midp=False, counts=False):
    """Exact Hardy-Weinberg p-value (see `hwe_exact_counts`) of every variant `ind_col` among the samples `ind_row`: one
    counting pass and the test on the device.  counts=True returns (p, the 4 x m counts of 0, 1, 2, missing) instead."""
    im, ir, ic = _ind(obj_bed, ind_row, ind_col)
    p = np.empty(ic.size)
    cnt = np.empty((ic.size, 4), dtype=np.int32) if counts else None
    check(_lib.load().bsn_bed_hwe(im.handle, ptr(ir, i64p), ir.size, ptr(ic, i64p), ic.size, int(bool(midp)), ptr(p, f64p),
                                  ptr(cnt, i32p)))
    return (p, cnt.T) if counts else p


def qc_classes(fam, founders_only=True, hwe_controls_only=True):
    """The class of every sample of a .fam table (a dict with paternal_ID, maternal_ID, affection) for bsn_bed_qc:
    0 = founder, counted for the Hardy-Weinberg test; 1 = founder, not counted for it; 2 = not a founder.  The rules are
    the module docstring's."""
    pat, mat = np.asarray(fam["paternal_ID"]).astype(str), np.asarray(fam["maternal_ID"]).astype(str)
    founder = (pat == "0") & (mat == "0") if founders_only else np.ones(pat.size, dtype=bool)
    cls = np.where(founder, 0, 2).astype(np.int32)
    if hwe_controls_only:
        try:
            aff = np.asarray(fam["affection"]).astype(np.float64)
        except ValueError:
            aff = None
        if aff is not None and np.isin(aff, (-9, 0, 1, 2)).all() and (aff == 1).any():
            cls[founder & (aff != 1)] = 1
    return cls


def autosomes(chromosome):
    """which entries of a .bim chromosome column are the integers 1 .. 22, after an optional 'chr' prefix"""
    out = np.zeros(len(chromosome), dtype=bool)
    for k, c in enumerate(np.asarray(chromosome).astype(str)):
        c = c[3:] if c[:3].lower() == "chr" else c
        out[k] = c.isdigit() and 1 <= int(c) <= 22
    return out


def _qc_call(im, ir, ic, cls, maf, geno, mind, hwe, midp):
    n, m = ir.size, ic.size
    keep_row, keep_col = np.empty(n, dtype=np.uint8), np.empty(m, dtype=np.uint8)
    row_miss, col_stats = np.empty(n), np.empty((m, 3))
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    check(_lib.load().bsn_bed_qc(im.handle, ptr(ir, i64p), n, ptr(ic, i64p), m, ptr(cls, i32p), float(maf), float(geno),
                                 float(mind), float(hwe), int(bool(midp)), ptr(keep_row, u8p), ptr(keep_col, u8p),
                                 ptr(row_miss, f64p), ptr(col_stats, f64p)))
    return keep_row.astype(bool), keep_col.astype(bool), row_miss, col_stats


def _x_of(im):
    from .plink_io import NAMES_FAM, NAMES_MAP, _read_table
    return dict(genotypes=im, fam=dict(zip(NAMES_FAM, _read_table(im.famfile, 6))),
                map=dict(zip(NAMES_MAP, _read_table(im.bimfile, 6))))


def _write_subset(im, bedfile_out, ind_row, ind_col):
    from .plink_io import snp_writeBed
    return snp_writeBed(_x_of(im), bedfile_out, ind_row=ind_row, ind_col=ind_col)


def _check_out(bedfile_out):
    bedfile_out = os.path.expanduser(str(bedfile_out))
    for f in (bedfile_out, sub_bed(bedfile_out, ".bim"), sub_bed(bedfile_out, ".fam")):
        if os.path.exists(f):
            raise FileExistsError("File '%s' already exists." % f)
    return bedfile_out


def bed_plinkQC(obj_bed, bedfile_out=None, maf=0.01, geno=0.1, mind=0.1, hwe=1e-50, autosome_only=False, founders_only=True,
                hwe_controls_only=True, midp=False, make_bed=True, ind_row=None, ind_col=None):
    """snp_plinkQC (R/external-software.R:247-290) without PLINK; the defaults and their meaning are the reference's.

    1. autosome_only keeps the variants whose .bim chromosome is an integer 1 .. 22 (an optional 'chr' prefix is
       dropped), before anything is counted.
    2. A sample is removed when more than `mind` of its genotypes over the selected variants are missing.
    3. Over the remaining samples, and independently of each other, a variant is removed when more than `geno` of its
       genotypes are missing, when its exact Hardy-Weinberg p-value (`hwe_exact_counts`; mid-p with midp=True) is below
       `hwe` (hwe=0 skips the test), or when its minor allele frequency is not at least `maf` (no genotype among the
       counted samples: removed whenever maf > 0).
    Which samples count for `maf` and `hwe` (founders; controls) is stated in the module docstring and `qc_classes`; an
    object without a .fam file counts every sample.

    make_bed=True writes the remaining samples and variants to `bedfile_out` (default "<in>_QC.bed") through snp_writeBed —
    which refuses to overwrite — and returns the path.  make_bed=False returns a report instead: keep_row / keep_col
    (bool, along ind_row / ind_col after the autosome filter), ind_row / ind_col (what is kept), row_miss (missing rate
    per sample), col_miss / maf / p_hwe (per variant, over the remaining samples) and `removed`, how many variants or
    samples each filter removes on its own (autosome, mind, geno, hwe, maf)."""
    im, ir, ic = _ind(obj_bed, ind_row, ind_col)
    has_files = bool(getattr(im, "bedfile", None))
    if make_bed:
        if not has_files:
            raise ValueError("bed_plinkQC(make_bed=True) needs a 'bed' object attached to a file (.bim and .fam are copied).")
        bedfile_out = _check_out(sub_bed(im.bedfile) + "_QC.bed" if bedfile_out is None else bedfile_out)
    n_before = ic.size
    if autosome_only:
        if not has_files:
            raise ValueError("bed_plinkQC(autosome_only=True) needs a 'bed' object attached to a file (the .bim is read).")
        ic = ic[autosomes(im.map["chromosome"])[ic]]
        if ic.size == 0:
            raise ValueError("bed_plinkQC: no autosomal variant is selected.")
    if has_files:
        cls = qc_classes(im.fam, founders_only, hwe_controls_only)[ir]
    else:
        cls = np.zeros(ir.size, dtype=np.int32)
    keep_row, keep_col, row_miss, stats = _qc_call(im, ir, ic, cls, maf, geno, mind, hwe, midp)
    if make_bed:
        if not keep_col.any():
            raise ValueError("bed_plinkQC: no variant passes the filters.")
        return _write_subset(im, bedfile_out, ir[keep_row], ic[keep_col])
    s1 = float(keep_row.sum())
    col_miss, maf_j, p = stats[:, 0].copy(), stats[:, 1].copy(), stats[:, 2].copy()
    with np.errstate(invalid="ignore"):
        removed = dict(autosome=int(n_before - ic.size), mind=int((~keep_row).sum()),
                       geno=int((np.rint(col_miss * s1) > float(geno) * s1).sum()),      # (the library's comparison: NA_j > geno |S1|)
                       hwe=int((p < hwe).sum()) if hwe > 0 else 0,
                       maf=int((~(maf_j >= maf)).sum()) if maf > 0 else 0)
    return dict(keep_row=keep_row, keep_col=keep_col, ind_row=ir[keep_row], ind_col=ic[keep_col], row_miss=row_miss,
                col_miss=col_miss, maf=maf_j, p_hwe=p, removed=removed)


def _pairs(df_or_files, col_family_ID, col_sample_ID, header):
    def column(table, col):
        if isinstance(table, dict):
            return list(table[col] if col in table else table[list(table)[col]])
        a = np.asarray(table)
        if a.ndim != 2:
            raise ValueError("'df_or_files' must be a table (a dict of columns, or rows) or a list of file paths.")
        return list(a[:, col])

    if isinstance(df_or_files, (str, os.PathLike)):
        df_or_files = [df_or_files]
    if isinstance(df_or_files, (list, tuple)) and df_or_files and all(isinstance(f, (str, os.PathLike)) for f in df_or_files):
        fid, iid = [], []
        for path in df_or_files:
            with open(os.path.expanduser(str(path))) as f:
                rows = [line.split() for line in f if line.strip()]
            for r in rows[1:] if header else rows:
                fid.append(r[col_family_ID]); iid.append(r[col_sample_ID])
        return fid, iid
    if isinstance(df_or_files, (dict, list, tuple, np.ndarray)):
        return column(df_or_files, col_family_ID), column(df_or_files, col_sample_ID)
    raise ValueError("'df_or_files' must be a table (a dict of columns, or rows) or a list of file paths.")


def bed_plinkRmSamples(obj_bed, bedfile_out, df_or_files, col_family_ID=0, col_sample_ID=1, header=False):
    """snp_plinkRmSamples (R/external-software.R:308-343) without PLINK: writes `bedfile_out` (.bed, .bim, .fam) without
    the samples named by (family ID, sample ID) pairs and returns its path.  `df_or_files` is a table — a dict of columns
    or a sequence of rows — or one or several paths of whitespace-separated files (header=True skips their first line);
    col_family_ID / col_sample_ID are 0-based positions (or keys of the dict).  A pair that is not in the .fam file is an
    error that names it; the file is written through snp_writeBed, which refuses to overwrite."""
    im, ir, ic = _ind(obj_bed, None, None)
    if not getattr(im, "bedfile", None):
        raise ValueError("bed_plinkRmSamples needs a 'bed' object attached to a file (.bim and .fam are copied).")
    bedfile_out = _check_out(bedfile_out)
    fid, iid = _pairs(df_or_files, col_family_ID, col_sample_ID, header)
    fam = im.fam
    where = {(str(f), str(s)): k for k, (f, s) in enumerate(zip(fam["family_ID"], fam["sample_ID"]))}
    gone = np.zeros(im.nrow, dtype=bool)
    for f, s in zip(fid, iid):
        k = where.get((str(f), str(s)))
        if k is None:
            raise ValueError("bed_plinkRmSamples: sample (family.ID '%s', sample.ID '%s') is not in '%s'." % (f, s, im.famfile))
        gone[k] = True
    if gone.all():
        raise ValueError("bed_plinkRmSamples: no sample would be left.")
    return _write_subset(im, bedfile_out, ir[~gone], ic)


def qc_last_ms():
    """device ms of the last bed_hwe / bed_plinkQC of this process: the per-sample counts, the per-class counting pass, the
    test kernel, the masks (bsn_qc_last_ms)"""
    ms = (C.c_double * 4)()
    check(_lib.load().bsn_qc_last_ms(ms))
    return [float(x) for x in ms]
