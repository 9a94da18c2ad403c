"""The statement of big_spLinReg / big_spLogReg on its own (tests/native/plr_ref.cpp over bigsnpr_amd/csrc/plr_step.hpp, DESIGN.md
3.5i), and the host logic of bigsnpr_amd/plr.py and snp_grid_stacking that needs no device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import plr_ref as ref  # noqa: E402
import plr_inputs as inp  # noqa: E402

PATH = inp.PATH


@pytest.fixture(scope="module")
def ex(orc, golden_dir, example_bed):
    return inp.example_case(orc, golden_dir, example_bed)


def _spread(f, r):
    """the discrete outputs of the two summation orders agree; returns max |d beta| / max |beta| and the relative spreads
    of intercept, loss and loss_val"""
    for k in ("status", "n_done", "best", "iter", "nb_active"):
        assert np.array_equal(f[k], r[k]), k
    assert np.array_equal(f["beta"] != 0, r["beta"] != 0)
    bmax = np.abs(f["beta"]).max()
    ok = ~np.isnan(f["loss"])
    assert np.array_equal(ok, ~np.isnan(r["loss"]))
    return (np.abs(f["beta"] - r["beta"]).max() / bmax, np.abs(f["intercept"] / r["intercept"] - 1).max(),
            np.abs(f["loss"][ok] / r["loss"][ok] - 1).max(), np.abs(f["loss_val"][ok] / r["loss_val"][ok] - 1).max())


@pytest.mark.parametrize("family", ["linear", "logistic"])
def test_two_summation_orders(ex, family):
    """forward and reversed row sums: every discrete output equal, beta within 1e-8 max|beta| (the measured spread is
    printed; tests/test_gpu_plr.py's tolerance is 1000 times it)"""
    y = ex["ylin"] if family == "linear" else ex["y01"]
    f = ref.fit(ex["X"], y, ex["fold"], 4, family=family, **PATH)
    r = ref.fit(ex["X"], y, ex["fold"], 4, family=family, reverse=True, **PATH)
    sb, si, sl, sv = _spread(f, r)
    nnz = (f["beta"] != 0).sum(axis=0)
    print("%s: spread of beta %.3g max|beta| (max|beta| = %.3g), intercept %.3g, loss %.3g, loss_val %.3g; status %s, "
          "n_done %s, best %s, non-zeros %s" % (family, sb, np.abs(f["beta"]).max(), si, sl, sv, f["status"], f["n_done"],
                                               f["best"], nnz))
    assert sb < 1e-8
    assert (f["best"] > 0).all() and (nnz > 0).all()       # the path did select something
    if family == "linear":
        assert set(f["status"]) == {1}                     # "No more improvement" on every fold


def _kkt(X, y, fold, k, a, lam, intercept, beta, family, pf=None):
    """the largest violation of the elastic-net optimality conditions on the training rows of fold k, in units of the
    bounds of the issue: (zero coefficients: |z| / (lambda a pf) - 1, others: |residual| / lambda)"""
    tr = fold != k
    Xt = X[tr]
    c, s = Xt.mean(axis=0), Xt.std(axis=0)
    live = s > 0
    eta = intercept + X @ beta
    g = (y - eta if family == "linear" else y - 1 / (1 + np.exp(-eta)))[tr]
    z = ((Xt[:, live] - c[live]) / s[live]).T @ g / tr.sum()
    b = (beta * s)[live]
    pf = np.ones(b.size) if pf is None else pf[live]
    zero = b == 0
    v0 = (np.abs(z[zero]) / (lam * a * pf[zero]) - 1).max() if zero.any() else -1.0
    v1 = (np.abs(z[~zero] - lam * a * pf[~zero] * np.sign(b[~zero]) - lam * (1 - a) * pf[~zero] * b[~zero])).max() / lam
    return v0, v1


@pytest.mark.parametrize("a", [1.0, 0.01])
@pytest.mark.parametrize("family", ["linear", "logistic"])
def test_kkt_at_the_last_lambda(ex, family, a):
    """eps = 1e-12 on a grid of 8 lambdas down to 0.5 lambda_max, which ends "Complete path" with the last lambda as
    the best one (the phenotypes carry enough signal for the validation loss to fall all the way): the returned model
    satisfies the optimality conditions, computed in numpy from the decoded matrix.  The stopping rule bounds the last
    pass's steps (shift^2 v < eps x null), not the gradient: the bound 1e-6 lambda holds where the last pass undershoots
    its threshold, as it does on a grid this shallow (a handful of nearly uncorrelated active columns); at 0.3 lambda_max
    the logistic chain of fold 1 stops at 1.9e-6 lambda, alpha = 1."""
    X, fold = ex["X"][:, :600], ex["fold"]
    y = ex["ystrong"] if family == "linear" else ex["y01strong"]
    f = ref.fit(X, y, fold, 4, alphas=[a], family=family, nlambda=8, lambda_min_ratio=0.5, nlam_min=8, n_abort=100,
                eps=1e-12, max_iter=100000)
    assert set(f["status"]) == {4}
    assert np.array_equal(f["best"], f["n_done"] - 1), (f["best"], f["loss_val"])
    for k in range(4):
        v0, v1 = _kkt(X, y, fold, k, a, f["lambda"][7, k], f["intercept"][k], f["beta"][:, k], family)
        print("%s, alpha %g, fold %d: zero coefficients |z| / bound - 1 = %.3g, others |residual| / lambda = %.3g, %d non-zero"
              % (family, a, k, v0, v1, (f["beta"][:, k] != 0).sum()))
        assert v0 <= 1e-6 and v1 <= 1e-6


def test_messages(ex):
    f = ref.fit(ex["X"], ex["ylin"], ex["fold"], 4, dfmax=20, **PATH)
    assert [ref.MESSAGES[s] for s in f["status"]] == ["Too many variables"] * 4
    assert (f["nb_active"][f["n_done"] - 1, np.arange(4)] >= 20).all()
    # a separable toy: column 0 decides y
    rng = np.random.default_rng(3)
    n = 120
    X = rng.standard_normal((n, 5))
    y = (X[:, 0] > 0).astype(np.float64)
    # (n_abort = 100: no early stop on the validation fold before the training deviance gets there)
    f = ref.fit(X, y, np.arange(n) % 3, 3, family="logistic", exact=False, nlambda=100, lambda_min_ratio=1e-4, n_abort=100)
    assert [ref.MESSAGES[s] for s in f["status"]] == ["Model saturated"] * 3
    assert np.isfinite(f["beta"]).all() and np.isfinite(f["loss_val"][f["n_done"] - 1, np.arange(3)]).all()


def _newton_logistic(Z, y):
    b = np.zeros(Z.shape[1])
    for _ in range(50):
        p = 1 / (1 + np.exp(-Z @ b))
        b = b + np.linalg.solve(Z.T @ (Z * (p * (1 - p))[:, None]), Z.T @ (y - p))
    return b


def test_unpenalised_covariates(ex):
    """pf_X = 1e12 on a grid that stays at lambda_max (lambda_min_ratio = 1: lambda_max is scaled by 1 / pf like every
    lambda, so only a grid that does not descend keeps the penalised columns out): the fit is the regression of y on
    [1, covar] over the training rows.  A monomorphic column and a single-column X give finite output, beta = 0 there."""
    rng = np.random.default_rng(5)
    n = ex["X"].shape[0]
    X = ex["X"][:, :40].copy()
    X[:, 7] = 1.0
    cov = rng.standard_normal((n, 3)) + 0.5 * ex["X"][:, [50]]
    fold = ex["fold"]
    pf = np.r_[np.full(40, 1e12), np.zeros(3)]
    kw = dict(covar=cov, pf=pf, nlambda=5, lambda_min_ratio=1.0, nlam_min=5, eps=1e-16, max_iter=100000)
    ylin = ex["ylin"] + cov @ np.array([0.5, -0.3, 0.2])
    y01 = (rng.random(n) < 1 / (1 + np.exp(-(cov @ np.array([1.0, -0.5, 0.3]) - 0.2)))).astype(np.float64)
    for family, y in (("linear", ylin), ("logistic", y01)):
        f = ref.fit(X, y, fold, 4, family=family, **kw)
        for k in range(4):
            tr = fold != k
            Z = np.column_stack([np.ones(tr.sum()), cov[tr]])
            want = np.linalg.lstsq(Z, y[tr], rcond=None)[0] if family == "linear" else _newton_logistic(Z, y[tr])
            got = np.r_[f["intercept"][k], f["beta"][40:, k]]
            print(family, k, np.abs(got - want).max(), np.abs(f["beta"][:40, k]).max())
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-8)
            assert np.abs(f["beta"][:40, k]).max() < 1e-8 and f["beta"][7, k] == 0
    # a single column; a single monomorphic column
    for x in (ex["X"][:, [3]], np.ones((n, 1))):
        for family, y in (("linear", ex["ylin"]), ("logistic", ex["y01"])):
            f = ref.fit(x, y, fold, 4, family=family, nlambda=10, nlam_min=3, n_abort=2)
            assert np.isfinite(f["beta"]).all() and np.isfinite(f["intercept"]).all() and (f["status"] > 0).all()
            if x[0, 0] == 1 and x.std() == 0:
                assert (f["beta"] == 0).all()


# ---- host logic ---------------------------------------------------------------------------------------------------------

def test_argument_checks_need_no_device():
    import bigsnpr_amd as ba
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((30, 8)), rng.standard_normal(30)
    y01 = (y > 0).astype(float)
    Xna = X.copy()
    Xna[3, 2] = np.nan
    with pytest.raises(ba.BsnError, match="You can't have missing values in 'X'.\n.*snp_fastImputeSimple"):
        ba.big_spLinReg(Xna, y)
    ba_err = ba.BsnError
    yna = y.copy()
    yna[0] = np.inf
    with pytest.raises(ba_err, match="missing values in 'y.train'"):
        ba.big_spLinReg(X, yna)
    with pytest.raises(ba_err, match="missing values in 'covar.train'"):
        ba.big_spLinReg(X, y, covar_train=np.full((30, 1), np.nan))
    with pytest.raises(ba_err, match="'y01.train' should be composed of 0s and 1s"):
        ba.big_spLogReg(X, y01 + 1)
    with pytest.raises(ba_err, match="'base.train' is not built"):
        ba.big_spLinReg(X, y, base_train=np.zeros(30))
    with pytest.raises(ba_err, match="not built"):
        ba.big_spLinReg(X, y, power_scale=0.5)
    with pytest.raises(ba_err, match="not built"):
        ba.big_spLogReg(X, y01, power_adaptive=1)
    with pytest.raises(ba_err, match="'K' must be at least 2"):
        ba.big_spLinReg(X, y, K=1)
    for bad in (0, 1.5, [1, -0.1]):
        with pytest.raises(ba_err, match=r"'alphas' must be in \(0, 1\]"):
            ba.big_spLinReg(X, y, alphas=bad)
    with pytest.raises(ba_err, match="should have the same length"):
        ba.big_spLinReg(X, y[:-1])
    with pytest.raises(TypeError, match="unexpected keyword"):
        ba.big_spLinReg(X, y, nonsense=1)
    s = ba.plr.draw_sets(103, 10, seed=1)
    assert s.dtype == np.int32 and np.array_equal(np.bincount(s), np.bincount(np.arange(103) % 10))
    assert np.array_equal(s, ba.plr.draw_sets(103, 10, seed=1)) and not np.array_equal(s, ba.plr.draw_sets(103, 10, seed=2))


def _fake_model(ba, family, n_covar=0):
    """two alphas x two folds with hand-made numbers over columns (4, 1, 6) of X"""
    mod = ba.BigSpReg()
    mod.family, mod.alphas, mod.ind_col, mod.n_covar = family, np.array([1.0, 0.5]), np.array([4, 1, 6]), n_covar
    p = 3 + n_covar
    for a, (lv, shift) in enumerate((([0.9, 0.7], 0.0), ([0.6, 0.5], 1.0))):
        mods = []
        for k in range(2):
            beta = np.r_[0.0, 1.0 + k + shift, -2.0, np.arange(1, n_covar + 1) * 0.5][:p]
            mods.append(dict(intercept=0.25 * (k + 1) + shift, beta=beta, loss_val=np.array([1.0, lv[k], 0.95]), best=1,
                             message="No more improvement" if k == 0 else "Complete path"))
        mod.append(mods)
    return mod


def test_summary_and_predict_on_a_dense_matrix():
    import bigsnpr_amd as ba
    rng = np.random.default_rng(1)
    X = rng.standard_normal((12, 8)).astype(np.float32)
    mod = _fake_model(ba, "binomial")
    rows = mod.summary()
    assert [r["alpha"] for r in rows] == [1.0, 0.5]
    assert rows[0]["validation_loss"] == pytest.approx(0.8) and rows[1]["validation_loss"] == pytest.approx(0.55)
    np.testing.assert_allclose(rows[0]["beta"], [0, 1.5, -2])
    assert rows[0]["intercept"] == pytest.approx(0.375) and rows[0]["nb_var"] == 2
    assert rows[0]["message"] == ["No more improvement", "Complete path"] and not rows[0]["all_conv"]
    best = mod.summary(best_only=True)
    assert len(best) == 1 and best[0]["alpha"] == 0.5
    want = 1.375 + X[:, [4, 1, 6]].astype(np.float64) @ np.array([0, 2.5, -2])
    np.testing.assert_allclose(mod.predict(X, proba=False), want, rtol=1e-14)
    np.testing.assert_allclose(mod.predict(X), 1 / (1 + np.exp(-want)), rtol=1e-14)
    sub = np.array([7, 2, 2])
    np.testing.assert_allclose(mod.predict(X, ind_row=sub, proba=False), want[sub], rtol=1e-14)
    lin = _fake_model(ba, "gaussian", n_covar=2)
    cov = rng.standard_normal((12, 2))
    np.testing.assert_allclose(lin.predict(X, covar_row=cov), want + cov @ np.array([0.5, 1.0]), rtol=1e-14)   # (proba is moot)
    with pytest.raises(ba.BsnError, match="'covar.row' is needed"):
        lin.predict(X)


def test_stacking_index_arithmetic():
    """stacking_coef against R/SCT.R:287-296 written out with R's 1-based indices, on a hand-made all_keep of two
    chromosomes with two sets each and three thresholds"""
    from bigsnpr_amd.sct import stacking_coef
    lpS = np.array([0.5, 2.5, 1.0, 3.5, 0.0, 1.5, 2.0])
    thr = np.array([0.4, 1.2, 2.2])
    all_keep = [[np.array([0, 2, 3]), np.array([1, 3])], [np.array([4, 5, 6]), np.array([6])]]
    rng = np.random.default_rng(2)
    beta_stacking = rng.standard_normal(12)
    # the transcription
    ind_last_thr = [1 + int(sum(lp > thr)) for lp in lpS]
    coef = [0.0] * len(lpS)
    n_thr = len(thr)
    ind = list(range(1, n_thr + 1))
    for ind_keep in [k + 1 for sets in all_keep for k in sets]:           # unlist(all_keep, recursive = FALSE), 1-based
        b = [beta_stacking[i - 1] for i in ind]
        b2 = [0.0] + list(np.cumsum(b))
        for j in ind_keep:
            coef[j - 1] = coef[j - 1] + b2[ind_last_thr[j - 1] - 1]
        ind = [i + n_thr for i in ind]
    np.testing.assert_allclose(stacking_coef(beta_stacking, lpS, thr, all_keep, 7), coef, rtol=1e-15)
    assert coef[4] == 0.0 and coef[3] != 0.0
