"""The BGEN files of tests/test_gpu_bgen_shapes.py, built the same way for tests/test_bgen_cpu.py, which proves without a
GPU that each of them reaches what it is there for in bigsnpr_amd/csrc/bgen.hip: the second turn of k_bgen_prod's loop
over kProdRows rows of Y, the second turn of k_bgen_grid8's stride over ind_row, repeated rows that draw different calls,
and the one sample whose probabilities add up to more than 1.  Every file comes from a fixed seed; and the rule the
products are held to, moved here unchanged from tests/test_gpu_bgen.py."""
import os
import sqlite3

import numpy as np

import bgen_inputs as bi

SEED = 20240611
PROD_ROWS, PROD_COLS = 128, 8          # kProdRows, kProdCols of bgen.hip
GRID8_THREADS = 1024 * 256             # k_bgen_grid8: at most 1 024 workgroups of 256, then the stride
MAX_NCOL = 65535 * PROD_COLS           # the grid's y at its limit


def check_product(got, X, beta):
    """|got - X beta| <= 4 m 2^-53 sum_j |x_ij| |beta_jc| per entry (the standard summation bound: both sides sum m
    products in fp64 in some order); NaN rows are exactly the samples with a missing value"""
    beta2 = beta[:, None] if beta.ndim == 1 else beta
    got2 = got[:, None] if got.ndim == 1 else got
    assert got2.shape == (X.shape[0], beta2.shape[1])
    nan_row = np.isnan(X).any(axis=1)
    assert np.array_equal(np.isnan(got2), np.repeat(nan_row[:, None], beta2.shape[1], axis=1))
    ok = ~nan_row
    want = X[ok] @ beta2
    bound = 4 * X.shape[1] * 2.0 ** -53 * (np.abs(X[ok]) @ np.abs(beta2))
    err = np.abs(got2[ok] - want)
    print("snp_prodBGEN: max error %.3g, max error / bound %.3g" % (err.max(initial=0.0), (err / np.maximum(bound, 1e-300)).max(initial=0.0)))
    assert (err <= bound).all()


def _written(path, p0, p1, miss, **kw):
    var = bi.write_bgen(path, p0, p1, miss, **kw)
    return dict(path=path, var=var, ids=[v["snp_id"] for v in var], offs=[v["offset"] for v in var], p0=p0, p1=p1,
                miss=miss, N=p0.shape[0], K=p0.shape[1])


def blocks(f):
    """the inflated blocks of a written file, variant by variant"""
    return [np.frombuffer(bi.inflated_block(f["p0"][:, j], f["p1"][:, j], f["miss"][:, j]), dtype=np.uint8)
            for j in range(f["K"])]


def case_ab(tmp):
    """A and B: 257 samples x 300 variants, so min(block_size, K) > kProdRows for block sizes 1000 (turns of 128, 128 and
    44 rows), 129 (a turn of one row; blocks of 129, 129, 42) and 256; B adds 7 (43 blocks, k0 = 7, 14 ...)"""
    p0, p1, miss = bi.probabilities(257, 300, seed=123, missing=0.001)
    f = _written(os.path.join(str(tmp), "ab.bgen"), p0, p1, miss)
    f.update(block_sizes_A=(1000, 129, 256), ncols_A=(8, 9, 16), block_sizes_B=(1000, 129, 7), ncol_B=9,
             rows_B=np.random.default_rng(31).integers(0, 257, 300), seed=SEED)
    f["beta_B"] = np.random.default_rng(32).integers(-3, 4, (300, 9)).astype(np.float64)
    return f


def case_c(tmp):
    """C: three files of 85 samples with 5, 1 and 130 variants: the third has a second turn at col0 = 6"""
    files = []
    for k, K in enumerate((5, 1, 130)):
        p0, p1, miss = bi.probabilities(85, K, seed=50 + k, missing=0.01)
        files.append(_written(os.path.join(str(tmp), "c%d.bgen" % k), p0, p1, miss, chrom="%02d" % (k + 1)))
    return dict(files=files, rows=np.random.default_rng(33).integers(0, 85, 120), seed=SEED + 7, block_size=1000,
                beta=np.random.default_rng(34).integers(-3, 4, (136, 9)).astype(np.float64))


def case_d(tmp):
    """D: 262 144 + 300 positions of ind_row: the 1 024 x 256 threads of k_bgen_grid8 take a second turn on the first 300"""
    p0, p1, miss = bi.probabilities(257, 3, seed=61, missing=0.02)
    f = _written(os.path.join(str(tmp), "d.bgen"), p0, p1, miss)
    f.update(rows=np.random.default_rng(35).integers(0, 257, GRID8_THREADS + 300), seed=SEED + 11)
    return f


def case_e(tmp, name="e"):
    """E: 21 x 7 in blocks of 2; sample 4 of variant 5 has (p0, p1) = (255, 1): 2 p0 + p1 = 511, one past the table.  The
    control has (255, 0) there: 510, the table's last entry."""
    p0, p1, miss = bi.probabilities(21, 7, seed=71, missing=0.05)
    miss[4, 5] = False
    p0[4, 5], p1[4, 5] = 255, 0
    good = _written(os.path.join(str(tmp), name + "_control.bgen"), p0, p1, miss, chrom="03")
    p1b = p1.copy()
    p1b[4, 5] = 1
    bad = _written(os.path.join(str(tmp), name + "_bad.bgen"), p0, p1b, miss, chrom="03")
    return dict(good=good, bad=bad, sample=4, variant=5, block=2, without=np.array([k for k in range(21) if k != 4] + [0, 20]))


def case_e_files(tmp):
    """E, second form: two good files, then E's bad file as the third"""
    files = []
    for k, K in enumerate((3, 2)):
        p0, p1, miss = bi.probabilities(21, K, seed=80 + k, missing=0.05)
        files.append(_written(os.path.join(str(tmp), "e3_%d.bgen" % k), p0, p1, miss, chrom="%02d" % (k + 1)))
    e = case_e(tmp, "e3")
    return dict(bad=files + [e["bad"]], good=files + [e["good"]])


def case_f(tmp):
    """F: one sample, one variant; beta of 1 x 524 280 columns fills blockIdx.y (65 535 tiles of 8), one more is refused"""
    f = _written(os.path.join(str(tmp), "f.bgen"), np.array([[100]], dtype=np.uint8), np.array([[31]], dtype=np.uint8),
                 np.array([[False]]))
    f.update(ncol=MAX_NCOL)
    return f


def case_g(tmp):
    """G: a good file, and a copy cut in the middle of its last record (with the same index)"""
    p0, p1, miss = bi.probabilities(21, 4, seed=91)
    f = _written(os.path.join(str(tmp), "g.bgen"), p0, p1, miss)
    raw = open(f["path"], "rb").read()
    last = f["var"][-1]
    cut = os.path.join(str(tmp), "g_cut.bgen")
    with open(cut, "wb") as h:
        h.write(raw[:last["offset"] + last["size"] // 2])
    with open(cut + ".bgi", "wb") as h:
        h.write(open(f["path"] + ".bgi", "rb").read())
    f.update(cut=cut, size=len(raw), cut_size=last["offset"] + last["size"] // 2, moved={})
    # ... and copies whose index puts the last record at the file's length and beyond it
    for name, off in (("at", len(raw)), ("beyond", len(raw) + 1000)):
        path = os.path.join(str(tmp), "g_%s.bgen" % name)
        with open(path, "wb") as h:
            h.write(raw)
        with open(path + ".bgi", "wb") as h:
            h.write(open(f["path"] + ".bgi", "rb").read())
        db = sqlite3.connect(path + ".bgi")
        db.execute("UPDATE Variant SET file_start_position = ? WHERE rsid = ?", (off, "rs%d" % (f["K"] - 1)))
        db.commit()
        db.close()
        f["moved"][name] = (path, off)
    return f
