"""snp_readBGEN / snp_prodBGEN — host mirror of R/read-bgen.R and R/prod-bgen.R over bsn_bgen_read / bsn_bgen_prod
(bigsnpr_amd/csrc/bgen.hip): the compressed probabilities go to the device as they lie in the file and are inflated and
decoded there.

What differs from the reference: the result of snp_readBGEN is an FBM_code256 with CODE_DOSAGE on the device (`.map`
beside it; no backing file is written, `.bytes` holds the FBM's bytes on request); read_as = "random" draws from the
library's counter-based generator keyed by `seed`, not from R's; indices are 0-based; `ncores` is accepted and dropped;
the index is read with the standard library's sqlite3.  Only what the reference reads is read: BGEN v1.2, layout 2,
zlib, two alleles, unphased, 8 bits per probability."""
import ctypes as C
import os
import re
import sqlite3
import struct

import numpy as np

from . import _lib
from ._lib import check, f64p, i64p, ptr, u8p, vp
from .ld import CODE_DOSAGE, FBM_code256

DECODE_BYTES = (207 - np.floor(np.arange(511) * 100 / 255 + 0.5)).astype(np.uint8)   # as.raw(207 - round(0:510 * 100 / 255))
DECODE_DOSAGE = np.arange(510, -1, -1) / 255                                        # 510:0 / 255
_BGI_COLUMNS = ("chromosome", "position", "rsid", "number_of_alleles", "allele1", "allele2", "file_start_position",
                "size_in_bytes")


def format_snp_id(snp_id):
    """R/read-bgen.R:4-9: two characters for the chromosome ("1_88169_C_T" -> "01_88169_C_T")"""
    out = [("0" + s) if s[1:2] == "_" else s for s in (str(s) for s in snp_id)]
    if any(s[2:3] != "_" for s in out):
        raise ValueError("Wrong format of some variants.")
    return out


def snp_readBGI(bgifile, snp_id=None):
    """Variant information from one .bgi index (R/read-bgen.R:26-63) as a dict of columns.  snp_id=None: all variants
    in the table's own order; else the rows that match the IDs "<chr>_<pos>_<a1>_<a2>", in the order of `snp_id`."""
    if not os.path.exists(bgifile):
        raise FileNotFoundError("File '%s' doesn't exist." % bgifile)
    db = sqlite3.connect("file:%s?mode=ro" % bgifile, uri=True)
    try:
        sql = "SELECT %s FROM Variant" % ", ".join(_BGI_COLUMNS)
        if snp_id is None:
            rows = db.execute(sql).fetchall()
        else:
            snp_id = format_snp_id(snp_id)
            pos = sorted({int(re.sub(r"^[0-9A-Za-z]{2}_([0-9]+)_.+$", r"\1", s)) for s in snp_id})
            rows = []
            for k in range(0, len(pos), 500):   # (the number of parameters of one statement is limited)
                part = pos[k:k + 500]
                rows += db.execute(sql + " WHERE position IN (%s)" % ", ".join("?" * len(part)), part).fetchall()
    finally:
        db.close()
    if snp_id is not None:
        first = {}
        for r, row in enumerate(rows):
            first.setdefault(format_snp_id(["%s_%s_%s_%s" % (row[0], row[1], row[4], row[5])])[0], r)   # match(): the first one
        ind = [first.get(s) for s in snp_id]
        if any(i is None for i in ind):
            missing = [s for s, i in zip(snp_id, ind) if i is None]
            raise ValueError("Some variants have not been found (e.g. '%s'; %d in all)." % (missing[0], len(missing)))
        rows = [rows[i] for i in ind]
    cols = list(zip(*rows)) if rows else [()] * len(_BGI_COLUMNS)
    out = {name: list(col) for name, col in zip(_BGI_COLUMNS, cols)}
    for name in ("position", "number_of_alleles", "file_start_position", "size_in_bytes"):
        out[name] = np.array(out[name], dtype=np.int64)
    return out


def check_bgen_format(bgenfile):
    """R/read-bgen.R:67-82: the number of samples of a BGEN file that is zlib-compressed and uses layout 2"""
    with open(bgenfile, "rb") as f:
        head = f.read(20)
        if len(head) < 20 or head[16:20] != b"bgen":
            raise ValueError("'%s' is not a BGEN file." % bgenfile)
        lh, = struct.unpack("<I", head[4:8])
        f.seek(4 + lh - 4)
        raw = f.read(4)
        if lh < 20 or len(raw) < 4:
            raise ValueError("'%s' is not a BGEN file." % bgenfile)
        flags, = struct.unpack("<I", raw)
    if flags & 3 != 1:
        raise ValueError("'%s' is not compressed with zlib." % bgenfile)
    if (flags >> 2) & 15 != 2:
        raise ValueError("'%s' is not using Layout 2." % bgenfile)
    return struct.unpack("<I", head[12:16])[0]


def _variant_ids(bgenfile, offsets):
    """the identifier (first string) of the records at `offsets`"""
    ids = []
    with open(bgenfile, "rb") as f:
        for off in offsets:
            f.seek(int(off))
            n, = struct.unpack("<H", f.read(2))
            ids.append(f.read(n).decode("utf-8", "replace"))
    return ids


def _check_args(bgenfiles, list_snp_id, ind_row, bgi_dir, read_as):
    if read_as not in ("dosage", "random"):
        raise ValueError("'read_as' should be one of \"dosage\", \"random\".")
    if isinstance(bgenfiles, (str, os.PathLike)):
        bgenfiles = [bgenfiles]
    bgenfiles = [os.path.expanduser(str(f)) for f in bgenfiles]
    for f in bgenfiles:
        if not f.endswith(".bgen"):
            raise ValueError("Extension of '%s' must be '.bgen'." % f)
    dirs = [os.path.dirname(f) for f in bgenfiles] if bgi_dir is None else (
        [str(bgi_dir)] * len(bgenfiles) if isinstance(bgi_dir, (str, os.PathLike)) else [str(d) for d in bgi_dir])
    bgifiles = [os.path.join(d, os.path.basename(f) + ".bgi") for d, f in zip(dirs, bgenfiles)]
    for f in bgenfiles + bgifiles:
        if not os.path.exists(f):
            raise FileNotFoundError("File '%s' doesn't exist." % f)
    if not isinstance(list_snp_id, list):
        raise TypeError("'list_snp_id' is not of class 'list'.")
    if any(s is None for ids in list_snp_id for s in ids):
        raise ValueError("You can't have missing values in 'list_snp_id'.")
    if len(list_snp_id) != len(bgenfiles):
        raise ValueError("Incompatibility between dimensions.\n'list_snp_id' and 'bgenfiles' should have the same length.")
    all_N = [check_bgen_format(f) for f in bgenfiles]
    if any(n != all_N[0] for n in all_N):
        raise ValueError("At least one value of 'all_N' is different from 'N'")
    N = int(all_N[0])
    ind_row = np.arange(N, dtype=np.int64) if ind_row is None else np.ascontiguousarray(ind_row, dtype=np.int64)
    if ind_row.size == 0 or ind_row.min() < 0 or ind_row.max() >= N:
        raise ValueError("all(ind_row >= 1 & ind_row <= N) is not TRUE")   # (0-based here: 0 .. N - 1)
    return bgenfiles, bgifiles, [len(ids) for ids in list_snp_id], N, ind_row


def _seed(seed):
    return int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & (2 ** 64 - 1)


def snp_readBGEN(bgenfiles, list_snp_id, ind_row=None, bgi_dir=None, read_as="dosage", ncores=1, seed=None,
                 return_bytes=False, block_variants=0):
    """The variants `list_snp_id` (one list of "<chr>_<pos>_<a1>_<a2>" per file) of the individuals `ind_row` as ONE
    FBM_code256 with CODE_DOSAGE on the device: dosages rounded to two decimal places, or hard calls drawn from the
    probabilities (read_as="random", keyed by `seed`).  `.map` holds chromosome, marker.ID, rsid, physical.pos, allele1,
    allele2, freq and info (R/read-bgen.R:213-216), `.bytes` (return_bytes=True) the FBM's bytes."""
    bgenfiles, bgifiles, sizes, N, ind_row = _check_args(bgenfiles, list_snp_id, ind_row, bgi_dir, read_as)
    seed = _seed(seed)
    n, m = int(ind_row.size), int(sum(sizes))
    if m == 0:
        raise ValueError("n and p must be positive.")
    lib = _lib.load()
    out = np.empty((n, m), dtype=np.uint8, order="F") if return_bytes else None
    info, freq = np.empty(m), np.empty(m)
    cols = {k: [] for k in ("chromosome", "marker.ID", "rsid", "physical.pos", "allele1", "allele2")}
    h, col0 = vp(), 0
    try:
        for bgen, bgi, ids, K in zip(bgenfiles, bgifiles, list_snp_id, sizes):
            if K == 0:
                continue
            tab = snp_readBGI(bgi, ids)
            offsets = np.ascontiguousarray(tab["file_start_position"], dtype=np.int64)
            check(lib.bsn_bgen_read(bgen.encode(), ptr(offsets, i64p), K, N, ptr(ind_row, i64p), n, ptr(DECODE_BYTES, u8p),
                                    int(read_as == "dosage"), seed, col0, m, int(block_variants), C.byref(h),
                                    None if out is None else C.cast(out.ctypes.data + col0 * n, u8p),
                                    C.cast(info.ctypes.data + 8 * col0, f64p), C.cast(freq.ctypes.data + 8 * col0, f64p)))
            cols["chromosome"] += tab["chromosome"]
            cols["marker.ID"] += _variant_ids(bgen, offsets)
            cols["rsid"] += tab["rsid"]
            cols["physical.pos"] += [int(p) for p in tab["position"]]
            cols["allele1"] += tab["allele1"]
            cols["allele2"] += tab["allele2"]
            col0 += K
    except Exception:
        if h.value:
            lib.bsn_bed_close(h)
        raise
    res = FBM_code256._from_handle(h, n, m, CODE_DOSAGE)
    cols["physical.pos"] = np.array(cols["physical.pos"], dtype=np.int64)
    cols["freq"], cols["info"] = freq, info
    res.map = cols
    res.seed = seed
    if return_bytes:
        res.bytes = out
    return res


def snp_prodBGEN(bgenfiles, beta, list_snp_id, ind_row=None, bgi_dir=None, read_as="dosage", block_size=1000, ncores=1,
                 seed=None):
    """bgen_data[ind_row, list_snp_id] %*% beta without an intermediate matrix (R/prod-bgen.R); the dosages are not
    rounded to two decimal places here.  A missing probability makes its individual's row NaN, as in the reference."""
    beta = np.asarray(beta, dtype=np.float64)
    is_vec = beta.ndim == 1
    if is_vec:
        beta = beta[:, None]
    if beta.ndim != 2:
        raise ValueError("'beta' should be a vector or a matrix.")
    bgenfiles, bgifiles, sizes, N, ind_row = _check_args(bgenfiles, list_snp_id, ind_row, bgi_dir, read_as)
    if beta.shape[0] != sum(sizes):
        raise ValueError("nrow(beta) == sum(sizes) is not TRUE")
    if int(block_size) < 1:
        raise ValueError("'block_size' should be at least 1.")
    seed = _seed(seed)
    n, ncol = int(ind_row.size), int(beta.shape[1])
    XY = np.zeros((n, ncol), order="F")
    if ncol == 0:
        return XY
    beta = np.asfortranarray(beta)
    lib = _lib.load()
    col0 = 0
    for bgen, bgi, ids, K in zip(bgenfiles, bgifiles, list_snp_id, sizes):
        if K == 0:
            continue
        offsets = np.ascontiguousarray(snp_readBGI(bgi, ids)["file_start_position"], dtype=np.int64)
        check(lib.bsn_bgen_prod(bgen.encode(), ptr(offsets, i64p), K, N, ptr(ind_row, i64p), n, ptr(DECODE_DOSAGE, f64p),
                                int(read_as == "dosage"), seed, col0, C.cast(beta.ctypes.data + 8 * col0, f64p), beta.shape[0],
                                ncol, int(block_size), ptr(XY, f64p)))
        col0 += K
    return XY[:, 0].copy() if is_vec else XY
