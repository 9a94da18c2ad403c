"""big_univLinReg / big_univLogReg on the device against the CPU statement (tests/native/gwas_ref.cpp, compiled from the
kernel's own irls_step.hpp) and, through the reference's PRS pipeline, against its golden files.

Tolerances (the ones the CPU statement holds against the oracle and numpy, tests/test_gwas_cpu.py): logistic
|d estim| <= 1e-9 std_err, std_err to 1e-7 relative, niter equal exactly; linear estim and std_err to 1e-7 relative."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

import gwas_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

THRS = np.arange(0, 5.5, 0.5)


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def _y01(golden_dir):
    return np.array([int(line.split()[5]) for line in open(os.path.join(golden_dir, "example.fam"))]) - 1.0


@pytest.fixture(scope="module")
def ex(ba, orc, golden_dir, example_bed):
    """the example data on the device and decoded on the host, the phenotype, 10 PCs, random covariates and a random
    normal phenotype; read-only"""
    X = np.asfortranarray(orc.read_bed(example_bed, na_val=3).astype(np.float64))
    rng = np.random.default_rng(2024)
    n = X.shape[0]
    return dict(X=X, n=n, m=X.shape[1], y=_y01(golden_dir), u=orc.dense_svd(example_bed, None, None, k=10)["u"],
                gb=ba.bed(os.path.join(golden_dir, "example.bed")), rnd=rng.standard_normal((n, 30)),
                ylin=rng.standard_normal(n) + 0.2 * X[:, 100], bytes=orc.fbm_from_bed(example_bed).bytes)


def _same_log(got, want, where=""):
    assert np.array_equal(got["niter"], want["niter"]), (where, np.flatnonzero(got["niter"] != want["niter"])[:10])
    nan = want["niter"] == 0
    assert np.isnan(got["estim"][nan]).all() and np.isnan(got["std_err"][nan]).all(), where
    assert np.isfinite(got["estim"][~nan]).all() and np.isfinite(got["std_err"][~nan]).all(), where
    ok = want["niter"] > 0                       # the values of niter = -1 variants are not compared
    d_est = np.abs(got["estim"][ok] - want["estim"][ok]) / want["std_err"][ok]
    d_se = np.abs(got["std_err"][ok] / want["std_err"][ok] - 1)
    print("%s: %d variants, max |d estim| / std_err = %.3g, max rel d std_err = %.3g, niter %d .. %d"
          % (where, ok.sum(), d_est.max(), d_se.max(), want["niter"][ok].min(), want["niter"][ok].max()))
    assert d_est.max() <= 1e-9, where
    assert d_se.max() <= 1e-7, where


def _same_lin(got, want, where=""):
    nan = np.isnan(want["estim"])
    assert np.isnan(got["estim"][nan]).all() and np.isnan(got["std_err"][nan]).all(), where
    d_est = np.abs(got["estim"][~nan] / want["estim"][~nan] - 1)
    d_se = np.abs(got["std_err"][~nan] / want["std_err"][~nan] - 1)
    print("%s: max rel d estim = %.3g, max rel d std_err = %.3g" % (where, d_est.max(), d_se.max()))
    assert d_est.max() <= 1e-7 and d_se.max() <= 1e-7, where
    assert got["df"] == want["df"]


def test_whole_example_data(ba, ex):
    """517 x 4542 with 10 covariates: P + 1 = 13, one accumulator tile"""
    got = ba.big_univLogReg(ex["gb"], ex["y"], covar_train=ex["u"])
    _same_log(got, ref.logreg(ex["X"], ex["y"], ex["u"]), "logistic, 10 PCs")
    np.testing.assert_allclose(got["score"], got["estim"] / got["std_err"])
    from scipy.stats import norm
    np.testing.assert_allclose(got["predict"](log10=False), 2 * norm.sf(np.abs(got["score"])), rtol=1e-10)
    lin = ba.big_univLinReg(ex["gb"], ex["ylin"], covar_train=ex["u"])
    _same_lin(lin, ref.linreg(ex["X"], ex["ylin"], ex["u"]), "linear, 10 PCs")
    from scipy.stats import t
    np.testing.assert_allclose(lin["predict"](log10=False), 2 * t.sf(np.abs(lin["score"]), lin["df"]), rtol=1e-10)
    np.testing.assert_allclose(lin["predict"](), np.log10(lin["predict"](log10=False)), rtol=1e-10)


@pytest.mark.parametrize("q", [0, 13, 14, 30])
def test_tile_edges(ba, ex, q):
    """P = 2; P + 1 = 16 fills one tile; 17 needs the second; q = 30 is the limit (z in a third operand tile)"""
    cols = np.arange(300)
    cov = ex["rnd"][:, :q] if q else None
    got = ba.big_univLogReg(ex["gb"], ex["y"], ind_col=cols, covar_train=cov)
    _same_log(got, ref.logreg(ex["X"][:, cols], ex["y"], cov), "logistic, q = %d" % q)
    lin = ba.big_univLinReg(ex["gb"], ex["ylin"], ind_col=cols, covar_train=cov)
    _same_lin(lin, ref.linreg(ex["X"][:, cols], ex["ylin"], cov), "linear, q = %d" % q)


@pytest.mark.parametrize("n_sub", [131, 263])
def test_row_and_column_lists(ba, ex, n_sub):
    """131 samples in shuffled order (no multiple of 4 or 64, less than one LDS tile), 263 (crosses one), and a
    non-contiguous column list whose length is no multiple of the four variants of a workgroup"""
    rng = np.random.default_rng(n_sub)
    rows = rng.permutation(ex["n"])[:n_sub]
    cols = np.sort(rng.choice(ex["m"], size=267, replace=False))
    y, cov = ex["y"][rows], ex["u"][rows]
    Xs = np.asfortranarray(ex["X"][np.ix_(rows, cols)])
    got = ba.big_univLogReg(ex["gb"], y, ind_train=rows, ind_col=cols, covar_train=cov)
    assert got["estim"].shape == (267,)
    _same_log(got, ref.logreg(Xs, y, cov), "logistic, %d rows" % n_sub)
    lin = ba.big_univLinReg(ex["gb"], ex["ylin"][rows], ind_train=rows, ind_col=cols, covar_train=cov)
    _same_lin(lin, ref.linreg(Xs, ex["ylin"][rows], cov), "linear, %d rows" % n_sub)


def test_dosage_image_of_the_same_calls(ba, ex):
    """CODE_DOSAGE bytes 7 + 100 g decode to 0.00 / 1.00 / 2.00: a byte image of the same calls"""
    cols = np.arange(500, 900)
    D = ba.FBM_code256((7 + 100 * ex["bytes"]).astype(np.uint8), code=ba.CODE_DOSAGE)
    assert D.bits == 8
    rows = np.random.default_rng(5).permutation(ex["n"])[:401]
    for ir in (None, rows):
        sel = slice(None) if ir is None else ir
        y, yl, cov = ex["y"][sel], ex["ylin"][sel], ex["u"][sel]
        a = ba.big_univLogReg(ex["gb"], y, ind_train=ir, ind_col=cols, covar_train=cov)
        b = ba.big_univLogReg(D, y, ind_train=ir, ind_col=cols, covar_train=cov)
        assert np.array_equal(a["niter"], b["niter"]) and (a["niter"] > 0).all()
        np.testing.assert_allclose(b["estim"], a["estim"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(b["std_err"], a["std_err"], rtol=1e-12, atol=0)
        a = ba.big_univLinReg(ex["gb"], yl, ind_train=ir, ind_col=cols, covar_train=cov)
        b = ba.big_univLinReg(D, yl, ind_train=ir, ind_col=cols, covar_train=cov)
        np.testing.assert_allclose(b["estim"], a["estim"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(b["std_err"], a["std_err"], rtol=1e-12, atol=0)


def _dosage_edges(ba):
    """333 x 44 random dosages: column 5 is 0.50 everywhere, column 6 is 2.00 everywhere, column 9 has a missing byte at
    sample 17.  (image, decoded matrix, y01, y, covariates, a permutation of the samples)"""
    rng = np.random.default_rng(21)
    n, m = 333, 44
    raw = rng.integers(7, 208, size=(n, m)).astype(np.uint8)
    raw[:, 5] = 57                               # dosage 0.50 everywhere
    raw[:, 6] = 207                              # 2.00 everywhere
    raw[17, 9] = 3                               # CODE_DOSAGE[3] is NA
    D = ba.FBM_code256(raw, code=ba.CODE_DOSAGE)
    assert D.bits == 8
    X = np.asfortranarray(ba.CODE_DOSAGE[raw])
    y, ylin, cov = (rng.random(n) < 0.5).astype(np.float64), rng.standard_normal(n), rng.standard_normal((n, 4))
    return D, X, y, ylin, cov, rng.permutation(n)


def test_dosage_image_edges(ba):
    """a byte image of real dosages against the CPU statement; a monomorphic column at a non-zero dosage and a column with
    a missing byte are NaN in both scans (niter = 0), over all samples and over a row list"""
    D, X, y, ylin, cov, perm = _dosage_edges(ba)
    for ir in (None, np.r_[17, perm[perm != 17][:200]]):     # (the list holds the sample with the missing byte)
        sel = slice(None) if ir is None else ir
        Xs = np.asfortranarray(X[sel])
        got = ba.big_univLogReg(D, y[sel], ind_train=ir, covar_train=cov[sel])
        assert list(got["niter"][[5, 6, 9]]) == [0, 0, 0] and np.isnan(got["estim"][[5, 6, 9]]).all()
        _same_log(got, ref.logreg(Xs, y[sel], cov[sel]), "logistic, dosages")
        lin = ba.big_univLinReg(D, ylin[sel], ind_train=ir, covar_train=cov[sel])
        assert np.isnan(lin["estim"][[5, 6, 9]]).all() and np.isnan(lin["std_err"][[5, 6, 9]]).all()
        _same_lin(lin, ref.linreg(Xs, ylin[sel], cov[sel]), "linear, dosages")


def test_missing_values(ba, orc, golden_dir, missing_bed):
    X = orc.read_bed(missing_bed, na_val=3).astype(np.float64)
    X[X == 3] = np.nan
    X = np.asfortranarray(X)
    n = X.shape[0]
    has_na = np.isnan(X).any(axis=0)
    assert has_na.any() and not has_na.all()
    rng = np.random.default_rng(11)
    y, ylin, cov = (rng.random(n) < 0.45).astype(np.float64), rng.standard_normal(n), rng.standard_normal((n, 3))
    gb = ba.bed(os.path.join(golden_dir, "example-missing.bed"))
    got, want = ba.big_univLogReg(gb, y, covar_train=cov), ref.logreg(X, y, cov)
    assert (got["niter"][has_na] == 0).all() and np.isnan(got["estim"][has_na]).all()
    assert np.isnan(got["std_err"][has_na]).all() and np.isnan(got["score"][has_na]).all()
    _same_log(got, want, "logistic, example-missing")
    lin = ba.big_univLinReg(gb, ylin, covar_train=cov)
    assert np.isnan(lin["estim"][has_na]).all() and np.isnan(lin["std_err"][has_na]).all()
    _same_lin(lin, ref.linreg(X, ylin, cov), "linear, example-missing")


def test_constructed_columns(ba, ex):
    g = np.array(ex["bytes"][:, :302], order="F")
    cases = np.flatnonzero(ex["y"] == 1)
    g[:, 300] = 1                                # monomorphic
    g[:, 301] = 0
    g[cases[:25], 301] = 1                       # carried only by cases: the likelihood has no maximum
    g[:, 7] = 0                                  # monomorphic at 0
    G = ba.FBM_code256(g)
    X = np.asfortranarray(g.astype(np.float64))
    got = ba.big_univLogReg(G, ex["y"], covar_train=ex["u"], verbose=False)
    want = ref.logreg(X, ex["y"], ex["u"])
    assert list(got["niter"][[7, 300, 301]]) == [0, 0, -1]
    assert np.isnan(got["estim"][[7, 300]]).all() and np.isnan(got["std_err"][[7, 300]]).all()
    assert np.isfinite(got["estim"][301]) and np.isfinite(got["std_err"][301])
    assert np.array_equal(np.flatnonzero(got["niter"] == -1), np.flatnonzero(want["niter"] == -1))
    _same_log(got, want, "logistic, constructed columns")
    lin = ba.big_univLinReg(G, ex["ylin"], covar_train=ex["u"])
    assert np.isnan(lin["estim"][[7, 300]]).all() and np.isfinite(lin["estim"][301])
    _same_lin(lin, ref.linreg(X, ex["ylin"], ex["u"]), "linear, constructed columns")


# ---- row lists and NaN rules in the other direction ---------------------------------------------------------------------------------

def _scan_both(ba, G, X, rows, cols, y, ylin, cov, where, **kw):
    """both scans over `rows` (and `cols`) against the CPU statement on that subset: (logistic, linear, statement of the
    logistic scan)"""
    Xs = np.asfortranarray(X[rows] if cols is None else X[np.ix_(rows, cols)])
    got = ba.big_univLogReg(G, y[rows], ind_train=rows, ind_col=cols, covar_train=None if cov is None else cov[rows], verbose=False, **kw)
    want = ref.logreg(Xs, y[rows], None if cov is None else cov[rows], **kw)
    _same_log(got, want, "logistic, " + where)
    lin = ba.big_univLinReg(G, ylin[rows], ind_train=rows, ind_col=cols, covar_train=None if cov is None else cov[rows])
    _same_lin(lin, ref.linreg(Xs, ylin[rows], None if cov is None else cov[rows]), "linear, " + where)
    return got, lin, want


def test_missing_value_outside_the_row_list(ba, orc, golden_dir, missing_bed):
    """variant 399 of example-missing.bed is missing at samples 17 and 71 only: over the other 198 samples it has a fit in
    both scans, while every variant with a missing value among them stays NaN.  The same on a byte image: the matrix of
    test_dosage_image_edges over a list without sample 17."""
    X = orc.read_bed(missing_bed, na_val=3).astype(np.float64)
    X[X == 3] = np.nan
    X = np.asfortranarray(X)
    n, j = X.shape[0], 399
    rows = np.flatnonzero(~np.isnan(X[:, j]))
    assert rows.size == n - 2 and list(np.flatnonzero(np.isnan(X[:, j]))) == [17, 71]
    still = np.isnan(X[rows]).any(axis=0)
    assert not still[j] and still.sum() > 300 and np.unique(X[rows, j]).size == 3
    rng = np.random.default_rng(11)
    y, ylin, cov = (rng.random(n) < 0.45).astype(np.float64), rng.standard_normal(n), rng.standard_normal((n, 3))
    gb = ba.bed(os.path.join(golden_dir, "example-missing.bed"))
    for order, ir in (("file order", rows), ("shuffled", rng.permutation(rows))):
        got, lin, want = _scan_both(ba, gb, X, ir, None, y, ylin, cov, "example-missing without samples 17 and 71, " + order)
        assert got["niter"][j] > 0 and np.isfinite(got["estim"][j]) and np.isfinite(got["std_err"][j])
        assert np.isfinite(lin["estim"][j]) and np.isfinite(lin["std_err"][j])
        assert (got["niter"][still] == 0).all() and np.isnan(got["estim"][still]).all() and np.isnan(lin["estim"][still]).all()
        assert np.isfinite(lin["estim"][~still]).sum() > 100                 # (a variant may be constant on the list)
    D, Xd, y, ylin, cov, perm = _dosage_edges(ba)
    for order, ir in (("file order", np.flatnonzero(np.arange(Xd.shape[0]) != 17)), ("a shuffled part", perm[perm != 17][:200])):
        got, lin, want = _scan_both(ba, D, Xd, ir, None, y, ylin, cov, "dosages without sample 17, " + order)
        assert got["niter"][9] > 0 and np.isfinite(got["estim"][9]) and np.isfinite(lin["estim"][9]) and np.isfinite(lin["std_err"][9])
        assert list(got["niter"][[5, 6]]) == [0, 0] and np.isnan(lin["estim"][[5, 6]]).all()
        assert (got["niter"][np.r_[0:5, 7:44]] != 0).all()


def test_constant_on_the_row_list_varying_outside(ba, ex):
    """a variant that is constant over ind_train and varies elsewhere has no fit: NaN and niter = 0 in both scans, on a
    2-bit image (code counts over the list) and on a byte image (n S2 = S1^2 over the list)"""
    n = ex["n"]
    rng = np.random.default_rng(77)
    perm = rng.permutation(np.arange(1, n))                  # sample 0 of the file stays outside the list
    rows, out = perm[:250], np.r_[0, perm[250:]]
    g = np.array(ex["bytes"][:, :40], order="F")
    g[rows, 10], g[out, 10] = 1, rng.integers(0, 3, out.size)        # constant 1 on the list, anything elsewhere
    g[:, 11] = 0
    g[0, 11] = 2                                                        # only sample 0 of the file differs: not in the list
    g[:, 12] = 2
    g[out[-1], 12] = 0                                                  # only one other sample outside the list differs
    g[:, 13] = 0
    g[rows[0], 13] = 1                                                  # varies on the list: only its FIRST row differs
    g[:, 14] = 1
    g[rows[-1], 14] = 2                                                 # ... only its last row
    const, single = [10, 11, 12], [13, 14]
    assert all(np.unique(g[rows, c]).size == 1 and np.unique(g[:, c]).size > 1 for c in const)
    assert all(np.unique(g[rows, c]).size == 2 for c in single) and 0 not in rows
    raw = (7 + 100 * g).astype(np.uint8)                                # the same calls as dosages 0.00 / 1.00 / 2.00 ...
    raw[:, 10] = np.where(np.isin(np.arange(n), rows), 57, rng.integers(7, 208, n))   # ... except 0.50 on the list
    raw[0, 11], raw[out[-1], 12] = 8, 206                               # and the smallest steps away from the constant
    D = ba.FBM_code256(raw, code=ba.CODE_DOSAGE)
    assert D.bits == 8
    for what, G, X in (("2-bit", ba.FBM_code256(g), g.astype(np.float64)), ("dosages", D, ba.CODE_DOSAGE[raw])):
        for order, ir in (("shuffled", rows), ("ascending", np.sort(rows))):
            got, lin, want = _scan_both(ba, G, X, ir, None, ex["y"], ex["ylin"], ex["u"][:, :3], "%s, %s list" % (what, order))
            assert list(got["niter"][const]) == [0, 0, 0] and list(want["niter"][const]) == [0, 0, 0]
            assert np.isnan(got["estim"][const]).all() and np.isnan(got["std_err"][const]).all()
            assert np.isnan(lin["estim"][const]).all() and np.isnan(lin["std_err"][const]).all()
            assert (got["niter"][single] != 0).all() and np.isfinite(lin["estim"][single]).all()


@pytest.mark.parametrize("q,n", [(3, 256), (3, 257), (14, 128), (14, 129), (0, 40), (0, 64), (0, 65),
                                 (15, 128), (15, 129), (30, 128), (30, 129)])
def test_sample_counts_at_the_tile_boundaries(ba, ex, q, n):
    """ind_train = the first n samples.  An LDS tile of k_logreg holds 256 samples when q + 2 <= 16 and 128 otherwise:
    (3, 256) fills one, (3, 257) starts a second with a single sample; (0, 40) is less than one step of 64
    samples, (0, 64) exactly one, (0, 65) one more.  q = 14 still takes the tile of 256 (q + 2 = 16), so (14, 128) and
    (14, 129) are two steps and two steps plus a sample of it; the tile of 128 starts at q = 15: (15, 128), (15, 129) and,
    with z in a third operand tile, (30, 128), (30, 129)."""
    rows, cols = np.arange(n), np.arange(300)
    cov = ex["rnd"][:, :q] if q else None
    assert q == 0 or np.linalg.matrix_rank(np.column_stack([np.ones(n), cov[:n]])) == q + 1
    got, lin, want = _scan_both(ba, ex["gb"], ex["X"], rows, cols, ex["y"], ex["ylin"], cov, "q = %d, first %d samples" % (q, n))
    assert (want["niter"] > 0).sum() > 250


@pytest.mark.parametrize("maxiter", [3, 4])
def test_workgroup_shapes(ba, ex, maxiter):
    """37 columns = nine workgroups of four variants and one with a single live wave.  The four variants of the first all
    stop at their first solve (two monomorphic, one with a missing value, one monomorphic at 2); with maxiter = 3 (4) some
    workgroup holds converged variants beside ones that end at -1, and the wave of the last workgroup ends on its own."""
    g = np.array(ex["bytes"][:, :40], order="F")
    g[:, 0], g[:, 1], g[5, 2], g[:, 3] = 1, 0, 3, 2
    cols = np.arange(37)
    G = ba.FBM_code256(g)
    X = g.astype(np.float64)
    X[g == 3] = np.nan
    rows = np.arange(ex["n"])
    got, lin, want = _scan_both(ba, G, X, rows, cols, ex["y"], ex["ylin"], ex["u"], "37 columns, maxiter = %d" % maxiter, maxiter=maxiter)
    assert cols.size % 4 == 1 and list(got["niter"][:4]) == [0, 0, 0, 0] and np.isnan(lin["estim"][:4]).all()
    groups = [set(np.sign(want["niter"][k:k + 4])) for k in range(4, 36, 4)]
    assert {1, -1} in groups, want["niter"]                              # converged and not converged in one workgroup
    assert want["niter"][36] != 0 and got["niter"][36] == want["niter"][36]
    last = want["niter"] == -1                                           # the last iterate of a variant that did not converge
    assert last.any() and (np.abs(got["estim"][last] - want["estim"][last]) <= 1e-9 * want["std_err"][last]).all()
    assert (np.abs(got["std_err"][last] / want["std_err"][last] - 1) <= 1e-7).all()


def test_maxiter_and_the_message(ba, ex, capsys):
    """one solve never converges (the variant's coefficient starts from 0): every fit is its last iterate, niter = -1"""
    cols = np.arange(40)
    got = ba.big_univLogReg(ex["gb"], ex["y"], ind_col=cols, covar_train=ex["u"], maxiter=1)
    want = ref.logreg(ex["X"][:, cols], ex["y"], ex["u"], maxiter=1)
    assert (got["niter"] == -1).all() and (want["niter"] == -1).all()
    assert "For 40 columns, IRLS didn't converge" in capsys.readouterr().out
    assert (np.abs(got["estim"] - want["estim"]) <= 1e-9 * want["std_err"]).all()


def test_linear_scan_is_multlinreg_for_one_pc(ba, ex):
    """two routes to one regression: the t-score of y = PC on x with an intercept"""
    for k in (0, 3):
        t = ba.multLinReg(ex["gb"], None, None, ex["u"][:, [k]])[:, 0]
        lin = ba.big_univLinReg(ex["gb"], ex["u"][:, k])
        assert lin["df"] == ex["n"] - 2
        np.testing.assert_allclose(lin["score"], t, rtol=1e-7, atol=0)


def test_refusals(ba, ex, golden_dir, monkeypatch):
    y = ex["y"]
    lut = ba.FBM_code256(ex["bytes"][:, :50], code=np.sqrt(np.arange(256.0)))
    for f, name in ((ba.big_univLogReg, "big_univLogReg"), (ba.big_univLinReg, "big_univLinReg")):
        with pytest.raises(ba.BsnError, match=name + " is not available for this FBM.code256"):
            f(lut, y)
    pitch = (ex["n"] + 3) // 4
    pitch = (pitch + 255) // 256 * 256
    monkeypatch.setenv("BSN_IMAGE_BUDGET", str(130 * pitch))
    ooc = ba.bed(os.path.join(golden_dir, "example.bed"))
    monkeypatch.delenv("BSN_IMAGE_BUDGET")
    assert ooc.streamed
    for f, name in ((ba.big_univLogReg, "big_univLogReg"), (ba.big_univLinReg, "big_univLinReg")):
        with pytest.raises(ba.BsnError, match=name + " needs the genotype image resident"):
            f(ooc, y)
    with pytest.raises(ba.BsnError, match="collinear"):
        ba.big_univLogReg(ex["gb"], y, ind_col=np.arange(8), covar_train=np.column_stack([ex["u"][:, 0], ex["u"][:, 0]]))


def test_the_pipeline_with_the_gwas_on_the_device(ba, orc, golden_dir, example_bed):
    """tests/test_prs_pipeline_golden.py's check (test-6-PRS.R:13-44) with `gwas` from big_univLogReg instead of the oracle:
    snp_autoSVD -> big_univLogReg -> snp_clumping -> snp_PRS, every genotype-touching step on the device"""
    G = ba.FBM_code256(orc.fbm_from_bed(example_bed).bytes)
    chrom, pos = orc.read_bim(os.path.join(golden_dir, "example.bed"))
    svd = ba.snp_autoSVD(G, chrom, pos, verbose=False)
    gwas = ba.big_univLogReg(G, _y01(golden_dir), covar_train=svd["u"])
    assert (gwas["niter"] > 0).all()
    pval = gwas["predict"](log10=False)
    pval2 = orc.read_rds(os.path.join(golden_dir, "pval.rds"))
    # expect_equal(pval, pval2, tolerance = 1e-4): mean relative difference
    assert np.mean(np.abs(pval - pval2)) / np.mean(np.abs(pval2)) < 1e-4
    keep = ba.snp_clumping(G, chrom, S=np.abs(gwas["score"]), size=250, infos_pos=pos)
    keep2 = orc.read_rds(os.path.join(golden_dir, "clumping.rds")) - 1
    assert np.isin(keep, keep2).mean() > 0.98
    lp = -np.log10(pval)

    def prs(b, keep, lp, thrs):
        return np.asarray(ba.snp_PRS(G, b, ind_keep=keep, lpS_keep=lp, thr_list=thrs))
    scores = prs(gwas["estim"][keep], keep, lp[keep], THRS)
    assert scores.shape == (G.nrow, THRS.size)
    prs2 = np.asarray(orc.read_rds(os.path.join(golden_dir, "scores-PRS.rds"))["value"]).reshape((G.nrow, THRS.size), order="F")
    cors = np.array([np.corrcoef(scores[:, j], prs2[:, j])[0, 1] for j in range(THRS.size)])
    np.testing.assert_allclose(cors, 1.0, atol=1e-3)
    # no ordering in `thrs` (test-6-PRS.R:46-57)
    perm = np.random.default_rng(0).permutation(THRS.size)
    scores_p = prs(gwas["estim"][keep], keep, lp[keep], THRS[perm])
    np.testing.assert_allclose(scores_p[:, np.argsort(perm)], scores, rtol=1e-12, atol=1e-12)
