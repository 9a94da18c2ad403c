"""big_spLinReg / big_spLogReg on the device against the CPU statement (tests/native/plr_ref.cpp, compiled from the kernels'
own plr_step.hpp), and snp_grid_stacking through the reference's test (tests/testthat/test-6-SCT.R:115-120).

Discrete outputs (message, number of lambdas, best index, passes per lambda, non-zeros per lambda, support) are equal
exactly.  beta (relative to max|beta|), intercept, loss and loss_val (relative to the value) are within 1000 x the spread
between the statement's forward and reversed row sums ON THAT INPUT, which every check measures and prints; the margin
covers a reduction tree that differs from both CPU orders.  A spread below one unit of fp64 rounding (2.2e-16) counts as
that: the device's tree is a third order, and a sum cannot be expected to agree better than its last bit.  The spreads
measured by tests/test_plr_cpu.py on the example data (517 x 1500, four folds, nlambda 60, nlam_min 15, n_abort 5):
    linear:   beta 1.2e-15 max|beta| (max|beta| 0.52), intercept 4.0e-15, loss 2.2e-15, loss_val 3.1e-15;
              "No more improvement" at l = 19 on every fold, best l = 11, 12, 10, 12 with 36, 30, 28, 16 non-zeros
    logistic: beta 1.6e-14 max|beta| (max|beta| 0.42), intercept 4.5e-14, loss 6.7e-15, loss_val 2.1e-15;
              "No more improvement" at l = 19, best l = 6, 5, 7, 6"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import plr_inputs as inp  # noqa: E402
import dosage_inputs as dos  # noqa: E402
from plr_check import _fit, _raw, _same  # noqa: E402

pytestmark = pytest.mark.gpu

PATH = inp.PATH


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def ex(ba, orc, golden_dir, example_bed):
    d = dict(inp.example_case(orc, golden_dir, example_bed))
    d["gb"] = ba.bed(os.path.join(golden_dir, "example.bed"))
    return d


@pytest.mark.parametrize("family", ["linear", "logistic"])
def test_example_data_on_the_2bit_image(ba, ex, family):
    """case 1: ind_col = 0 .. 1499 of the whole image (a compacted copy of the columns), four folds"""
    y = ex["ylin"] if family == "linear" else ex["y01"]
    mod = _fit(ba, family, ex["gb"], y, ind_col=np.arange(inp.N_COL), ind_sets=ex["fold"], **PATH)
    f = _same(mod, ex["X"], y, ex["fold"], 4, family + ", example data", family=family, **PATH)
    assert (f["best"] > 0).all()
    assert mod.family == ("gaussian" if family == "linear" else "binomial") and len(mod) == 1 and len(mod[0]) == 4
    assert mod[0][2]["ind_col"].size == inp.N_COL and mod[0][2]["alpha"] == 1.0
    best = mod.summary(best_only=True)[0]
    np.testing.assert_allclose(best["beta"], f["beta"].mean(axis=1), rtol=0, atol=1e-11)


@pytest.mark.parametrize("family", ["linear", "logistic"])
def test_row_list_strided_columns_and_covariates(ba, ex, family):
    """case 2: an unsorted ind_train of 401 rows, every third column, three unpenalised covariates"""
    rng = np.random.default_rng(12)
    rows = rng.permutation(517)[:401]
    cols = np.arange(2, inp.N_COL, 3)
    cov = rng.standard_normal((401, 3))
    y = (ex["ylin"] if family == "linear" else ex["y01"])[rows] + (cov[:, 0] if family == "linear" else 0)
    fold = ex["fold"][rows]
    mod = _fit(ba, family, ex["gb"], y, ind_train=rows, ind_col=cols, covar_train=cov, pf_covar=np.zeros(3), ind_sets=fold,
               **PATH)
    Xs = np.asfortranarray(ex["X"][np.ix_(rows, cols)])
    f = _same(mod, Xs, y, fold, 4, family + ", 401 rows", family=family, covar=cov, **PATH)
    assert (f["beta"][cols.size:] != 0).all() and mod.n_covar == 3
    # predict on the image: the averaged model through bed_prodVec
    best = mod.summary(best_only=True)[0]
    want = best["intercept"] + Xs @ best["beta"][:cols.size] + cov @ best["beta"][cols.size:]
    got = mod.predict(ex["gb"], ind_row=rows, covar_row=cov, proba=False)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(want).max())


def test_dosage_byte_image(ba):
    """case 3: CODE_DOSAGE, 2051 x 300: more than two turns of the sweep's 1024-thread row loop, n no multiple of 4 or 64;
    column 11 is constant, column 12 constant on the training rows of fold 1 only"""
    rng = np.random.default_rng(31)
    n, m = 2051, 300
    k = rng.integers(-100, 101, size=(n, m)).astype(np.int8)
    k[:, 1] = np.clip(k[:, 0] + rng.integers(-20, 21, n), -100, 100)      # a correlated pair
    k[:, 11] = 37
    fold = rng.permutation(np.arange(n) % 3).astype(np.int32)
    k[:, 12] = np.where(fold == 1, k[:, 12], -5)
    raw = dos.dosage_bytes(k)
    D = ba.FBM_code256(raw, code=ba.CODE_DOSAGE)
    assert D.bits == 8
    X = np.asfortranarray(ba.CODE_DOSAGE[raw])
    lin = X[:, [0, 40, 80, 120]] @ np.array([0.8, -0.6, 0.5, 0.7])
    kw = dict(nlambda=40, nlam_min=10, n_abort=4)
    for family, y in (("linear", lin + rng.standard_normal(n)), ("logistic", (rng.random(n) < 1 / (1 + np.exp(-(lin - lin.mean())))).astype(float))):
        mod = _fit(ba, family, D, y, ind_sets=fold, **kw)
        f = _same(mod, X, y, fold, 3, family + ", dosages", family=family, **kw)
        assert (f["beta"][11] == 0).all() and f["beta"][12, 1] == 0 and (f["best"] > 0).all()


@pytest.mark.parametrize("family", ["linear", "logistic"])
@pytest.mark.parametrize("dtype,order", [(np.float32, "C"), (np.float32, "F"), (np.float64, "C"), (np.float64, "F")])
def test_dense_matrix(ba, ex, dtype, order, family):
    """case 4: 517 x 700, float32 and float64, C- and F-ordered"""
    rng = np.random.default_rng(41)
    A = (ex["X"][:, :700] + 0.25 * rng.standard_normal((517, 700))).astype(np.float32)
    A = np.asarray(A.astype(dtype), order=order)
    assert A.flags["C_CONTIGUOUS" if order == "C" else "F_CONTIGUOUS"]
    kw = dict(nlambda=40, nlam_min=10, n_abort=4)
    y = ex["ylin"] if family == "linear" else ex["y01"]
    mod = _fit(ba, family, A, y, ind_sets=ex["fold"], **kw)
    _same(mod, A.astype(np.float64), y, ex["fold"], 4, "%s dense %s %s" % (family, np.dtype(dtype).name, order),
          family=family, exact=False, **kw)
    np.testing.assert_allclose(mod.predict(A, proba=False)[:5], (mod.summary(True)[0]["intercept"] + A.astype(np.float64)
                                                                 @ mod.summary(True)[0]["beta"])[:5], rtol=1e-12)


@pytest.mark.parametrize("family", ["linear", "logistic"])
@pytest.mark.parametrize("how", ["entering", "covariate"])
def test_one_active_column_over_several_passes(ba, ex, family, how):
    """A chain whose active set is a single column for more than one pass, alpha = 0.5: every thread of the sweep has to see
    the coefficient that thread 0 stored in the previous pass, and a linear chain with one column has no reduction of
    another column in between.  517 rows leave seven of the sixteen waves without a row.  "entering": one column carries
    the phenotype, so it is alone in the set over the first lambdas of a shallow grid; "covariate": the start fit of one
    unpenalised covariate."""
    rng = np.random.default_rng(61)
    cols = np.arange(300)
    X = np.asfortranarray(ex["X"][:, :300])
    x = (X[:, 10] - X[:, 10].mean()) / X[:, 10].std()
    kw = dict(alphas=[0.5], nlambda=6, lambda_min_ratio=0.8, nlam_min=6, n_abort=6)
    cov = None
    if how == "covariate":
        cov = rng.standard_normal((517, 1))
        lin = 1.5 * cov[:, 0] + 0.3 * x
    else:
        lin = 1.5 * x
    y = lin + 0.5 * rng.standard_normal(517) if family == "linear" else (rng.random(517) < 1 / (1 + np.exp(-lin))).astype(float)
    mod = _fit(ba, family, ex["gb"], y, ind_col=cols, covar_train=cov, ind_sets=ex["fold"], **kw)
    f = _same(mod, X, y, ex["fold"], 4, "%s, one active column (%s)" % (family, how), family=family, covar=cov, **kw)
    alone = (f["nb_active"] == 1) & (f["iter"] >= 2)
    assert alone[0].all() if how == "covariate" else alone[1:3].all(), (f["nb_active"], f["iter"])


def test_thirty_chains_in_lockstep(ba, ex):
    """case 5: 10 folds x 3 alphas in one call, nlambda 40: the loop carries finished and live chains together"""
    rng = np.random.default_rng(51)
    fold = rng.permutation(np.arange(517) % 10).astype(np.int32)
    cols = np.arange(500)
    alphas = [1, 0.5, 0.05]
    kw = dict(nlambda=40, nlam_min=8, n_abort=3)
    mod = _fit(ba, "linear", ex["gb"], ex["ylin"], ind_col=cols, ind_sets=fold, alphas=alphas, **kw)
    f = _same(mod, np.asfortranarray(ex["X"][:, :500]), ex["ylin"], fold, 10, "30 chains", alphas=alphas, **kw)
    assert len(mod) == 3 and all(len(m) == 10 for m in mod)
    assert np.unique(f["n_done"]).size >= 2, f["n_done"]
    rows = mod.summary()
    assert [r["alpha"] for r in rows] == [1.0, 0.5, 0.05] and len(mod.summary(best_only=True)) == 1


def test_dfmax_and_complete_path(ba, ex):
    """case 6"""
    cols = np.arange(inp.N_COL)
    with pytest.warns(UserWarning, match="Too many variables"):
        mod = ba.big_spLinReg(ex["gb"], ex["ylin"], ind_col=cols, ind_sets=ex["fold"], dfmax=20, **PATH)
    assert [mo["message"] for mo in mod[0]] == ["Too many variables"] * 4
    _same(mod, ex["X"], ex["ylin"], ex["fold"], 4, "dfmax 20", dfmax=20, **PATH)
    kw = dict(nlambda=8, lambda_min_ratio=0.5, nlam_min=8, n_abort=100)
    for family, y in (("linear", ex["ystrong"]), ("logistic", ex["y01strong"])):
        mod = _fit(ba, family, ex["gb"], y, ind_col=cols[:600], ind_sets=ex["fold"], **kw)
        assert [mo["message"] for mo in mod[0]] == ["Complete path"] * 4 and all(mo["lambda"].size == 8 for mo in mod[0])
        _same(mod, np.asfortranarray(ex["X"][:, :600]), y, ex["fold"], 4, family + ", complete path", family=family, **kw)


def test_two_identical_calls_are_bit_equal(ba, ex):
    """case 7"""
    cols = np.arange(0, inp.N_COL, 2)
    for family, y in (("linear", ex["ylin"]), ("logistic", ex["y01"])):
        a, b = (_raw(_fit(ba, family, ex["gb"], y, ind_col=cols, ind_sets=ex["fold"], alphas=[1, 0.1], **PATH)) for _ in range(2))
        for k in ("intercept", "beta", "n_done", "best", "status"):
            assert np.array_equal(a[k], b[k]), (family, k)
        for k in ("loss", "loss_val", "iter", "nb_active"):
            assert all(np.array_equal(u, v) for u, v in zip(a[k], b[k])), (family, k)


def test_refusals(ba, ex, golden_dir, monkeypatch):
    """case 8"""
    gm = ba.bed(os.path.join(golden_dir, "example-missing.bed"))
    y = np.random.default_rng(0).standard_normal(gm.nrow)
    for f, yy in ((ba.big_spLinReg, y), (ba.big_spLogReg, (y > 0).astype(float))):
        with pytest.raises(ba.BsnError, match="You can't have missing values in 'X'.\n.*snp_fastImputeSimple"):
            f(gm, yy, K=4, seed=1)
    pitch = (517 + 3) // 4
    pitch = (pitch + 255) // 256 * 256
    monkeypatch.setenv("BSN_IMAGE_BUDGET", str(130 * pitch))
    ooc = ba.bed(os.path.join(golden_dir, "example.bed"))
    monkeypatch.delenv("BSN_IMAGE_BUDGET")
    assert ooc.streamed
    for f, name, yy in ((ba.big_spLinReg, "big_spLinReg", ex["ylin"]), (ba.big_spLogReg, "big_spLogReg", ex["y01"])):
        with pytest.raises(ba.BsnError, match=name + " needs the genotype image resident"):
            f(ooc, yy, K=4, seed=1)


def test_stacking_mirrors_the_reference_test(ba, orc, ex, example_bed, golden_dir):
    """test-6-SCT.R:115-120: snp_grid_clumping -> snp_grid_PRS (thresholds 0:5) -> snp_grid_stacking(alphas = 1e-3)"""
    G = ba.FBM_code256(orc.fbm_from_bed(example_bed).bytes)
    rng = np.random.default_rng(6)
    CHR = np.repeat([1, 2], [2542, 2000])
    POS = orc.read_bim(os.path.join(golden_dir, "example.bed"))[1]
    lpval = -np.log10(rng.uniform(size=G.ncol))
    betas = rng.normal(0, 0.1, G.ncol)
    all_keep = ba.snp_grid_clumping(G, CHR, POS, lpval, grid_thr_r2=(0.05, 0.2, 0.8), grid_base_size=(100, 200))
    multi_PRS = ba.snp_grid_PRS(G, all_keep, betas, lpval, grid_lpS_thr=np.arange(6.0))
    assert multi_PRS.shape == (517, 72)
    new_betas = ba.snp_grid_stacking(multi_PRS, ex["y01"], alphas=1e-3, ind_sets=rng.permutation(np.arange(517) % 10))
    assert new_betas["beta_covar"].size == 0 and new_betas["mod"].family == "binomial"
    assert np.count_nonzero(new_betas["beta_G"]) > 0
    pred = new_betas["mod"].predict(multi_PRS, proba=False)
    want = new_betas["intercept"] + ba.big_prodVec(G, new_betas["beta_G"])
    # expect_equal(..., tolerance = 1e-6): mean relative difference
    assert np.mean(np.abs(pred - want)) / np.mean(np.abs(want)) < 1e-6
    lin = ba.snp_grid_stacking(multi_PRS, ex["ylin"], alphas=1e-3, K=5, seed=3)
    assert lin["mod"].family == "gaussian"
