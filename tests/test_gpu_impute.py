"""snp_fastImputeSimple on the device (bsn_impute_simple, bigsnpr_amd/csrc/impute.hip) against the CPU statement
(tests/native/impute_ref.cpp, compiled from the same impute_step.hpp).  Everything is bytes and integers: every
comparison is an equality, on example-missing.bed, on shapes at the edges of the image layout, on the rounding and
mode-tie variants, for `random` bit for bit; the result handle is the image bsn_fbm_open makes of the same bytes; the
source stays untouched; the FBM entry points that refuse missing values run on the result."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import impute_ref as ref  # noqa: E402
from impute_inputs import METHODS, SEED, check_edges, column, edge_matrix, impute, same_image  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def ex(golden_dir):
    """example-missing.bed as FBM bytes and what the CPU statement makes of it under every method (computed once)"""
    G = ref.read_bed_bytes(os.path.join(golden_dir, "example-missing.bed"), 200, 500)
    return dict(path=os.path.join(golden_dir, "example-missing.bed"), G=G,
                want={me: ref.impute(G, me, seed=SEED)[0] for me in METHODS})


# ---- 1. example data, all five methods ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_example_data(ba, ex, method):
    for src in (ba.bed(ex["path"]), ba.FBM_code256(ex["G"])):
        if method == "zero":
            with pytest.warns(UserWarning, match="deprecated"):
                res = ba.snp_fastImputeSimple(src, "zero", seed=SEED, return_bytes=True)
        else:
            res = ba.snp_fastImputeSimple(src, method, seed=SEED, return_bytes=True)
        assert np.array_equal(res.bytes, ex["want"][method])
        assert res.n_all_missing == 0 and not res._has_na and res.seed == SEED and res.shape == (200, 500)
        assert res.bits == (8 if method == "mean2" else 2)
        table = {"zero": np.array([0, 1, 2, 0] + [np.nan] * 252), "mean2": ba.CODE_DOSAGE}.get(method, ba.CODE_IMPUTE_PRED)
        assert np.array_equal(res.code256, table, equal_nan=True)
        # the reference's expectations (test-3-fastImpute.R:117-130, 1-based there), read back through the result
        c400, c1 = column(ba, res, 399), column(ba, res, 0)
        if method == "zero":
            assert list(c400[[17, 71]]) == [0, 0]
        elif method in ("mean0", "mode"):
            assert list(c400[[17, 71]]) == [1, 1]
        elif method == "mean2":
            assert list(c400[[17, 71]]) == [101, 101]
        if method == "mode":
            assert list(c1[[3, 11]]) == [0, 0]
        # decoded sums: what the calls and the imputed values add up to (in hundredths: exact integers)
        dec = np.where(ex["G"] < 3, ex["G"] * 100, 0).astype(np.int64)
        b = res.bytes.astype(np.int64)
        dec += np.where(ex["G"] == 3, {"zero": 0 * b, "mean2": b - 7}.get(method, (b - 4) * 100), 0)
        assert np.array_equal(np.rint(100 * ba.snp_colstats(res)["sumX"]).astype(np.int64), dec.sum(0))
        # the source still decodes the two positions as missing
        im = src if isinstance(src, ba.bed) else src._bed
        assert list(ba.read_bed(im, np.array([17, 71]), np.array([399]))[:, 0]) == [-1, -1]


# ---- 2. the result handle is the image bsn_fbm_open would make ----------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_result_is_the_image_of_its_bytes(ba, ex, method):
    same_image(ba, impute(ba, ba.FBM_code256(ex["G"]), method, seed=SEED, return_bytes=True))


# ---- 3. shapes at the edges of the layout -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 17, 1025])
@pytest.mark.parametrize("method", METHODS)
def test_shapes_at_the_edges(ba, n, method):
    check_edges(ba, edge_matrix(n, 65), method)
    for kind in range(4):   # m = 1: complete, all missing, first sample only, last sample only
        col = np.random.default_rng(n + kind).integers(0, 3, (n, 1)).astype(np.uint8)
        if kind == 1:
            col[:] = 3
        elif kind == 2:
            col[0] = 3
        elif kind == 3:
            col[n - 1] = 3
        check_edges(ba, np.asfortranarray(col), method)


# ---- 4. rounding and mode-tie variants -----------------------------------------------------------------------------------------
def test_rounding_and_mode_ties(ba):
    """columns of 44 samples: c observed calls with c1 + 2 c2 = s, the rest missing"""
    n = 44
    cols, exp = [], {"mean2": {}, "mean0": {}, "mode": {}}

    def add(c0, c1, c2):
        cols.append([0] * c0 + [1] * c1 + [2] * c2 + [3] * (n - c0 - c1 - c2))
        return len(cols) - 1
    # (c, s) -> r: 100 * (s / c) in fp64, ties to even (57.49999999999999, 122.50000000000001, 127.49999999999999, 12.5, 62.5)
    exp["mean2"][add(17, 23, 0)] = 7 + 57
    exp["mean2"][add(0, 31, 9)] = 7 + 123
    exp["mean2"][add(0, 29, 11)] = 7 + 127
    exp["mean2"][add(7, 1, 0)] = 7 + 12
    exp["mean2"][add(5, 1, 2)] = 7 + 62
    exp["mean0"][add(1, 1, 0)] = 4 + 0    # 0.5
    exp["mean0"][add(0, 1, 1)] = 4 + 2    # 1.5
    exp["mode"][add(4, 4, 2)] = 4 + 0     # c0 == c1 > c2
    exp["mode"][add(2, 4, 4)] = 4 + 1     # c1 == c2 > c0
    exp["mode"][add(4, 2, 4)] = 4 + 0     # c0 == c2 > c1
    exp["mode"][add(3, 3, 3)] = 4 + 0     # all three equal
    g = np.asfortranarray(np.array(cols, dtype=np.uint8).T)
    G = ba.FBM_code256(g)
    for method, want in exp.items():
        res = impute(ba, G, method, return_bytes=True)
        for j, byte in want.items():
            assert (res.bytes[g[:, j] == 3, j] == byte).all(), (method, j, byte, res.bytes[-1, j])
        assert np.array_equal(res.bytes, ref.impute(g, method)[0])
        same_image(ba, res)


# ---- 5. random --------------------------------------------------------------------------------------------------------------
def test_random(ba):
    col = ref.chi_square_column()
    g = np.asfortranarray(np.stack([col, col], axis=1))
    G = ba.FBM_code256(g)
    res = impute(ba, G, "random", seed=SEED, return_bytes=True)
    assert np.array_equal(res.bytes, ref.impute(g, "random", seed=SEED)[0])       # bit-equal to the CPU statement
    again = impute(ba, G, "random", seed=SEED, return_bytes=True)
    assert np.array_equal(again.bytes, res.bytes)                                  # the same seed, the same bytes
    other = impute(ba, G, "random", seed=SEED + 1, return_bytes=True)
    assert not np.array_equal(other.bytes, res.bytes)
    plain = impute(ba, G, "random", seed=SEED)                                     # independent of return_bytes
    assert not hasattr(plain, "bytes")
    np.testing.assert_array_equal(plain._bed.download(), res._bed.download())
    same_image(ba, res)
    na = col == 3
    assert not np.array_equal(res.bytes[na, 0], res.bytes[na, 1])                  # two variants, two sets of draws
    for j in (0, 1):
        pv = ref.chi_square_pvalue(col, res.bytes[:, j])
        print("variant", j, "p-value", pv)
        assert pv > 1e-4
    fresh = impute(ba, G, "random"), impute(ba, G, "random")                      # seed=None: a fresh key, kept on the result
    assert fresh[0].seed != fresh[1].seed
    np.testing.assert_array_equal(impute(ba, G, "random", seed=fresh[0].seed)._bed.download(), fresh[0]._bed.download())


# ---- 6. the source is untouched -----------------------------------------------------------------------------------------------
def test_source_untouched(ba, ex):
    for src in (ba.bed(ex["path"]), ba.FBM_code256(ex["G"])):
        im = src if isinstance(src, ba.bed) else src._bed
        before, counts = im.download(), ba.bed_counts(im)
        for method in METHODS:
            impute(ba, src, method, seed=SEED, return_bytes=(method == "mode"))
            np.testing.assert_array_equal(im.download(), before)
            np.testing.assert_array_equal(ba.bed_counts(im), counts)


# ---- 7. the point of the feature ---------------------------------------------------------------------------------------------------
def test_fbm_entry_points_run_on_the_result(ba, ex):
    """The products and the partial SVD of an FBM refuse missing values and point at this function; snp_cor (pairwise
    complete) and big_univLinReg (NaN for such variants) accept them.  On the imputed FBM all of them run and agree with
    the same call on an FBM uploaded from the CPU statement's bytes."""
    G = ba.FBM_code256(ex["G"])
    rng = np.random.default_rng(11)
    x, y = rng.standard_normal(500), rng.standard_normal(200)
    for call in (lambda: ba.big_randomSVD(G, k=5), lambda: ba.big_prodVec(G, x), lambda: ba.big_cprodVec(G, y)):
        with pytest.raises(ValueError, match="impute first \\(snp_fastImputeSimple\\)"):
            call()
    has_na = (ex["G"] == 3).any(0)
    assert np.isnan(ba.big_univLinReg(G, y)["estim"][has_na]).all()
    G2 = impute(ba, G, "mode")
    twin = ba.FBM_code256(ex["want"]["mode"], ba.CODE_IMPUTE_PRED)
    a, b = ba.big_randomSVD(G2, k=5), ba.big_randomSVD(twin, k=5)
    # the same integer products on identical images from the same start: what is left is the order of fp64 sums
    np.testing.assert_allclose(a["d"], b["d"], rtol=1e-10)
    assert a["d"].shape == (5,) and np.all(np.isfinite(a["d"])) and np.all(a["d"] > 0)
    ca, cb = ba.snp_cor(G2, size=50), ba.snp_cor(twin, size=50)
    np.testing.assert_array_equal(ca.p, cb.p)
    np.testing.assert_array_equal(ca.i, cb.i)
    np.testing.assert_array_equal(ca.x, cb.x)
    la, lb = ba.big_univLinReg(G2, y), ba.big_univLinReg(twin, y)
    np.testing.assert_array_equal(la["estim"], lb["estim"])
    np.testing.assert_array_equal(la["std_err"], lb["std_err"])
    mono = np.array([np.unique(c).size == 1 for c in np.where(ex["want"]["mode"] > 3, ex["want"]["mode"] - 4, ex["want"]["mode"]).T])
    assert np.isfinite(la["estim"][~mono]).all()
    np.testing.assert_array_equal(ba.big_prodVec(G2, x), ba.big_prodVec(twin, x))
    np.testing.assert_array_equal(ba.big_cprodVec(G2, y), ba.big_cprodVec(twin, y))


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(ba, ex, golden_dir, monkeypatch):
    from bigsnpr_amd import _lib
    L = _lib.load()
    # a byte image (the host mirror stops at its table first: asked of the library itself)
    D = ba.FBM_code256(np.where(ex["G"] < 3, ex["G"] + 4, 3).astype(np.uint8), ba.CODE_DOSAGE)
    assert D.bits == 8
    h, n_all = C.c_void_p(), C.c_int64(0)
    assert L.bsn_impute_simple(D.handle, 1, 0, C.byref(h), None, C.byref(n_all)) != 0
    assert "2-bit genotype image" in L.bsn_last_error().decode() and "snp_fastImputeSimple" in L.bsn_last_error().decode()
    G = ba.FBM_code256(ex["G"])
    assert L.bsn_impute_simple(G.handle, 5, 0, C.byref(h), None, None) != 0
    assert "'method' should be" in L.bsn_last_error().decode()
    # an out-of-core source
    res = ba.bed(ex["path"])
    pitch = (res.nrow + 3) // 4 + 255 & ~255
    monkeypatch.setenv("BSN_IMAGE_BUDGET", str(130 * pitch))
    ooc = ba.bed(ex["path"])
    monkeypatch.delenv("BSN_IMAGE_BUDGET")
    assert ooc.streamed
    with pytest.raises(ba.BsnError, match="snp_fastImputeSimple needs the genotype image resident"):
        ba.snp_fastImputeSimple(ooc)
    # a wrong table, a wrong method
    with pytest.raises(ValueError, match="CODE_012"):
        ba.snp_fastImputeSimple(ba.FBM_code256(ex["want"]["mode"], ba.CODE_IMPUTE_PRED))
    with pytest.raises(ValueError, match="should be one of"):
        ba.snp_fastImputeSimple(ba.FBM_code256(ex["G"]), "mean")
    with pytest.raises(TypeError, match="not of class"):
        ba.snp_fastImputeSimple(ex["G"])
