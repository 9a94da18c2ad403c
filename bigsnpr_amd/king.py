"""bed_king / bed_kingQC — the KING-robust kinship table and the removal of related samples, host mirror of
snp_plinkKINGQC (R/external-software.R:520-590) over bsn_bed_king (bigsnpr_amd/csrc/king.hip).

The reference hands this step to a PLINK 2 child process (--make-king-table / --king-cutoff).  Here the table is computed
on the device from the handle's 2-bit image: five exact counts per pair of samples and the between-family estimator of
Manichaikul et al. 2010, as PLINK 2 documents them for --make-king-table.

PLINK 2's own --king-cutoff selection of the samples to remove is NOT emulated: it is not specified beyond "prune one of
each related pair", and no PLINK binary exists here to pin it against.  `king_norel` states the rule used instead, in
full; it reproduces what the reference's test expects of example.bed (tests/testthat/test-3-plink-QC.R:90-114: `POP1
IND2` removed)."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import check, f64p, i32p, i64p, ptr, vp
from .bed import sub_bed
from .ld import _ind

COUNT_NAMES = ("NSNP", "HETHET", "IBS0", "HET1HOM2", "HET2HOM1")


def _table(im, ir, ic, thr, filt):
    lib = _lib.load()
    h, count = vp(), C.c_int64(0)
    check(lib.bsn_bed_king(im.handle, ptr(ir, i64p), ir.size, ptr(ic, i64p), ic.size, float(thr), int(filt), C.byref(count),
                           C.byref(h)))
    try:
        k = int(count.value)
        i1, i2 = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32)
        counts, kin = np.empty((k, 5), dtype=np.int32), np.empty(k)
        check(lib.bsn_king_fetch(h, ptr(i1, i32p), ptr(i2, i32p), ptr(counts, i32p), ptr(kin, f64p)))
    finally:
        lib.bsn_king_free(h)
    res = dict(I1=i1, I2=i2)
    for q, name in enumerate(COUNT_NAMES):
        res[name] = np.ascontiguousarray(counts[:, q])
    res["KINSHIP"] = kin
    return res


def bed_king(obj_bed, thr_king=None, ind_row=None, ind_col=None):
    """The KING-robust table of the pairs of samples `ind_row` over the variants `ind_col`: a dict of arrays, one entry
    per pair, ascending in (I1, I2).

    I1 < I2 are positions in `ind_row` (0-based; any list, repeats included).  Over the variants where both samples are
    called: NSNP, HETHET (both heterozygous), IBS0 (opposite homozygotes), HET1HOM2 (the first heterozygous, the second
    homozygous), HET2HOM1 (the reverse), and
        KINSHIP = 0.5 - (4 IBS0 + HET1HOM2 + HET2HOM1) / (4 (HETHET + min(HET1HOM2, HET2HOM1)))
    — NaN for 0 / 0, -inf for any other zero denominator.  thr_king = None returns every pair, non-finite ones included;
    a number keeps the pairs with KINSHIP >= thr_king (PLINK 2's --king-table-filter).  FID1, IID1, FID2, IID2 are added
    when the object has a .fam file."""
    im, ir, ic = _ind(obj_bed, ind_row, ind_col)
    res = _table(im, ir, ic, 0.0 if thr_king is None else thr_king, thr_king is not None)
    if getattr(im, "bedfile", None):
        fam = im.fam
        for name, col, idx in (("FID1", "family_ID", "I1"), ("IID1", "sample_ID", "I1"), ("FID2", "family_ID", "I2"),
                               ("IID2", "sample_ID", "I2")):
            res[name] = fam[col][ir[res[idx]]]
    return res


def king_norel(table, n):
    """The samples to keep so that no pair of `table` (a dict with I1 and I2, positions below n) remains: while pairs
    remain, remove the sample that occurs in the most remaining pairs, ties toward the LARGER index.  Returns (keep,
    removed): ascending positions kept, positions removed in the order of removal.  Runs on the host; PLINK 2's own
    --king-cutoff selection is not emulated (see the module's docstring)."""
    i1 = np.asarray(table["I1"], dtype=np.int64).ravel()
    i2 = np.asarray(table["I2"], dtype=np.int64).ravel()
    if i1.size != i2.size:
        raise ValueError("Incompatibility between dimensions.\n'I1' and 'I2' should have the same length.")
    n = int(n)
    if i1.size and (min(i1.min(), i2.min()) < 0 or max(i1.max(), i2.max()) >= n):
        raise IndexError("'table' names a sample outside 0 .. n - 1.")
    alive = i1 != i2
    deg = np.bincount(i1[alive], minlength=n) + np.bincount(i2[alive], minlength=n)
    removed = []
    while alive.any():
        top = int(n - 1 - np.argmax(deg[::-1]))       # the largest index among the most connected
        hit = alive & ((i1 == top) | (i2 == top))
        deg -= np.bincount(i1[hit], minlength=n) + np.bincount(i2[hit], minlength=n)
        alive &= ~hit
        removed.append(top)
    keep = np.setdiff1d(np.arange(n, dtype=np.int64), np.array(removed, dtype=np.int64))
    return keep, np.array(removed, dtype=np.int64)


def bed_kingQC(obj_bed, thr_king=2 ** -3.5, make_bed=True, bedfile_out=None, ind_row=None, ind_col=None):
    """snp_plinkKINGQC (R/external-software.R:520-590) without PLINK: thr_king as there (0.354 screens duplicates and
    twins, 0.177 first-degree relations as well, 0.0884 — the default — second-degree ones as well).

    make_bed=False: the table of the pairs with KINSHIP >= thr_king (bed_king).  make_bed=True: writes the samples that
    `king_norel` keeps (all variants `ind_col`) to `bedfile_out`, default "<in>_norel.bed", through snp_writeBed — which
    refuses to overwrite — and returns the path.  `extra.options` has no counterpart; PLINK 2's own selection of the
    samples to remove is not emulated (king_norel is the rule, it reproduces the reference's test expectation)."""
    if not make_bed:
        return bed_king(obj_bed, thr_king, ind_row, ind_col)
    im, ir, ic = _ind(obj_bed, ind_row, ind_col)
    if not getattr(im, "bedfile", None):
        raise ValueError("bed_kingQC(make_bed=True) needs a 'bed' object attached to a file (.bim and .fam are copied).")
    if bedfile_out is None:
        bedfile_out = sub_bed(im.bedfile) + "_norel.bed"
    bedfile_out = os.path.expanduser(str(bedfile_out))
    for f in (bedfile_out, sub_bed(bedfile_out, ".bim"), sub_bed(bedfile_out, ".fam")):
        if os.path.exists(f):
            raise FileExistsError("File '%s' already exists." % f)
    table = _table(im, ir, ic, thr_king, True)
    keep, _ = king_norel(table, ir.size)
    from .plink_io import NAMES_FAM, NAMES_MAP, _read_table, snp_writeBed
    x = dict(genotypes=im, fam=dict(zip(NAMES_FAM, _read_table(im.famfile, 6))),
             map=dict(zip(NAMES_MAP, _read_table(im.bimfile, 6))))
    return snp_writeBed(x, bedfile_out, ind_row=ir[keep], ind_col=ic)


def king_last_ms():
    """device ms of the last bed_king / bed_kingQC of this process: the operand (gathered selection, sample-major copy),
    the per-sample totals of the two-product path (0 on the general path), the pair kernel, the compaction
    (bsn_king_last_ms)"""
    ms = (C.c_double * 4)()
    check(_lib.load().bsn_king_last_ms(ms))
    return [float(x) for x in ms]
