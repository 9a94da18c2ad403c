"""The byte-image kernels (bsn_bed::bits == 8) past one int32 accumulator slice: more than 131 072 samples.

Windowed LD cuts the samples into slices (k_pair_xy8 + k_band_fill8) or splits no longer than one (k_pair_stats8 +
k_band_fill8na); the products (k_cprod8 / k_prod8) contract over 132 352 samples, the smallest pitch at which one int32 per
digit column is not enough.  Inputs and references: tests/helpers/dosage_inputs.py — exact integer sums, the reference's
expressions (src/corr.cpp:54-86, src/ld-scores.cpp) in np.longdouble; tests/test_dosage_inputs_cpu.py shows without a GPU
that a wrong slice, a dropped or doubled slice or a wrapped accumulator cannot pass on them.  Tolerances are those of the
byte-image tests in tests/test_gpu_fbm.py: 1e-9 absolute on r, 1e-9 relative on LD scores, identical sparsity pattern,
identical clumping, products within 1e-9 of the largest reference entry."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dosage_inputs as di  # noqa: E402
from test_gpu_fbm import _close  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = 40
ALPHA = 0.05


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def panel():
    return di.slice_panel()


def _check_cor(ba, orc, G, sums, pos, rows, **kw):
    got = ba.snp_cor(G, ind_row=rows, size=SIZE, infos_pos=pos, **kw)
    thr = orc.cor_thresholds(sums.n, kw.get("alpha", 1.0), kw.get("thr_r2", 0.0))
    ri, rp, rx, margin = di.cor_reference(sums, pos, SIZE, thr)
    print("snp_cor %s rows=%d: %d entries, nearest |r| to its threshold %.2e, max |x - ref| %s"
          % (kw, sums.n, rx.size, margin, np.abs(got.x - rx).max() if got.x.size == rx.size else "(sizes differ)"))
    assert margin > 1e-7
    np.testing.assert_array_equal(got.p, rp)
    np.testing.assert_array_equal(got.i, ri)
    np.testing.assert_allclose(got.x, rx, rtol=0, atol=1e-9)
    return got


def _check_ld_scores(ba, G, sums, pos, rows):
    got, ref = ba.snp_ld_scores(G, ind_row=rows, size=SIZE, infos_pos=pos), di.ld_scores_reference(sums, pos, SIZE)
    print("snp_ld_scores rows=%d: max relative difference %.2e" % (sums.n, np.abs(got / ref - 1).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-9)


# ---- windowed LD ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def grid_fbm(ba, panel):
    G = ba.FBM_code256(di.grid255_bytes(panel[0]), di.GRID255)
    assert G.bits == 8 and not G._has_na and di.pitch_of(G.nrow) > di.SLICE
    return G


@pytest.mark.parametrize("rows", ["all", "subset"])
def test_complete_data_across_two_slices(ba, orc, panel, grid_fbm, rows):
    """k_pair_xy8 + k_band_fill8 with nslice = 2: the cross product of the saturated twins passes 2^31 over the row and fits
    an int32 only per slice; the second slice flips the sign of half the correlations"""
    k, pos = panel
    ir = None if rows == "all" else di.slice_rows()
    sums = di.PairSums(k, rows=ir)
    got = _check_cor(ba, orc, grid_fbm, sums, pos, ir, thr_r2=0.1)
    st = ba.ld.last_stats()
    assert "cross product only" in st["kernel"] and st["products"] == 1
    # the twins: r from 2 180 640 800 = sum of 135 300 products of +-127 (all rows)
    j0, j = di.TWINS[1], di.TWINS[0]
    col = slice(got.p[j0], got.p[j0 + 1])
    assert got.i[col][0] == j and abs(got.x[col][0] - float(sums.r()[0][j0, j])) < 1e-9
    _check_cor(ba, orc, grid_fbm, sums, pos, ir, alpha=ALPHA)
    _check_ld_scores(ba, grid_fbm, sums, pos, ir)
    assert "cross product only" in ba.ld.last_stats()["kernel"]


def test_clumping_and_value_units_across_two_slices(ba, orc, panel):
    """the same panel on CODE_DOSAGE's grid (v_off = 1, v_step = 0.01): mode 2 of k_band_fill8 maps the sliced cross product
    to value units; the kept variants are the oracle's, with and without ind_row; r and the LD scores as above, r against the
    oracle's scalar loop too"""
    k, pos = panel
    kd = di.dosage_indices(k)
    raw = di.dosage_bytes(kd)
    G, Go = ba.FBM_code256(raw, ba.CODE_DOSAGE), orc.FBM256(raw, ba.CODE_DOSAGE)
    assert G.bits == 8 and not G._has_na
    np.testing.assert_array_equal(ba.CODE_DOSAGE, di.CODE_DOSAGE)
    chrom = np.repeat([1, 2], [100, di.SLICE_M - 100])
    ir = di.slice_rows()
    for rows in (None, ir):
        np.testing.assert_array_equal(ba.snp_clumping(G, chrom, thr_r2=0.2, infos_pos=pos, ind_row=rows),
                                      orc.snp_clumping(Go, chrom, thr_r2=0.2, infos_pos=pos, ind_row=rows))
    assert "cross product only" in ba.ld.last_stats()["kernel"]
    kept = ba.snp_clumping(G, chrom, thr_r2=0.2, infos_pos=pos)
    assert 10 < kept.size < di.SLICE_M - 10
    sums = di.PairSums(kd)
    _check_ld_scores(ba, G, sums, pos, None)
    got = _check_cor(ba, orc, G, sums, pos, None, thr_r2=0.1)
    oi, op_, ox = orc.snp_cor(Go, size=SIZE, infos_pos=pos, thr_r2=0.1)
    np.testing.assert_array_equal(got.p, op_)
    np.testing.assert_array_equal(got.i, oi)
    np.testing.assert_allclose(got.x, ox, rtol=0, atol=1e-9)


@pytest.mark.parametrize("rows", ["all", "subset"])
def test_missing_values_with_splits_beyond_one_slice(ba, orc, panel, rows):
    """k_pair_stats8 + k_band_fill8na: three tile-pair rows of a 135 424-byte pitch take splits over both slices, their int32
    sums added into int64 statistics; pairwise-complete sums from masked matmuls"""
    k, pos = panel
    miss = di.slice_missing()
    G = ba.FBM_code256(di.grid255_bytes(k, miss), di.GRID255)
    assert G.bits == 8 and G._has_na
    ir = None if rows == "all" else di.slice_rows()
    sums = di.PairSums(k, miss, rows=ir)
    _check_cor(ba, orc, G, sums, pos, ir, thr_r2=0.1)
    assert "8 products" in ba.ld.last_stats()["kernel"]
    _check_cor(ba, orc, G, sums, pos, ir, alpha=ALPHA)
    _check_ld_scores(ba, G, sums, pos, ir)
    assert "8 products" in ba.ld.last_stats()["kernel"]


def test_windowed_ld_refuses_a_seventh_slice(ba):
    n = di.MAX_SLICES * di.SLICE + 1
    G = ba.FBM_code256(np.full((n, 2), 130, dtype=np.uint8), di.GRID255)
    assert G.bits == 8
    with pytest.raises(ba.BsnError, match="at most 786432 samples"):
        ba.snp_cor(G, size=10)


# ---- products -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def over_fbm(ba):
    G = ba.FBM_code256(di.grid255_bytes(di.overflow_panel()), di.GRID255)
    assert G.bits == 8 and not G._has_na and G.nrow == di.OVER_N
    return G


def _vector(case):
    rng = np.random.default_rng(12)
    n, m = di.OVER_N, di.OVER_M
    cols = center = scale = None
    if case == "digits -128 and 126":
        y = np.full(n, di.OVER_Y)
    elif case == "ones":
        y = np.ones(n)
    else:
        y = rng.normal(size=n)
    if case == "centre and scale":
        center, scale = rng.normal(size=m), rng.uniform(0.5, 2.0, size=m)
    if case == "column subset":
        cols = np.array([0, 1, 2, 5, 6, 9, 40, 41, 77, 100, 128, 129])
        y = np.full(n, di.OVER_Y)
    return y, cols, center, scale


@pytest.mark.parametrize("case", ["digits -128 and 126", "ones", "random", "centre and scale", "column subset"])
def test_cprod_at_132352_samples(ba, over_fbm, case):
    """k_cprod8 over 517 chunks of 256 samples: y = 32128 has the digits [0, 0, 0, 0, 0, -128, 126] at every sample, so the
    -128 column of variant 0 (127 throughout) sums to -2 151 514 112 < -2^31 — two slices keep it exact"""
    k = di.overflow_panel()
    y, cols, center, scale = _vector(case)
    got = ba.big_cprodVec(over_fbm, y, None, cols, center, scale)
    ref = di.cprod_reference(k, y, cols, center, scale)
    err = np.abs(got - ref)
    print("big_cprodVec, %s: max |z - ref| = %.3e at variant %d (z = %.17g, ref = %.17g), largest |ref| = %.3e"
          % (case, err.max(), err.argmax(), got[err.argmax()], ref[err.argmax()], np.abs(ref).max()))
    _close(got, ref)


def test_prod_at_132352_samples(ba, over_fbm):
    """k_prod8 at 517 workgroups along the samples"""
    x = np.random.default_rng(13).normal(size=di.OVER_M)
    _close(ba.big_prodVec(over_fbm, x), di.prod_reference(di.overflow_panel(), x))


def test_products_refuse_a_seventh_slice(ba):
    """the crossproduct keeps one int32 partial sum per slice for at most six slices, like windowed LD: the next size says so"""
    n = di.MAX_SLICES * di.SLICE + 1
    G = ba.FBM_code256(np.full((n, 16), 130, dtype=np.uint8), di.GRID255)
    assert G.bits == 8
    with pytest.raises(ba.BsnError, match="at most 786432 samples"):
        ba.big_cprodVec(G, np.ones(n))
