"""snp_lassosum2 on the device against the CPU statement of src/lassosum2.cpp (tests/native/lassosum2_ref.c): bit for bit.
The LD matrix is bed_cor of tests/golden/example.bed on the device; the summary statistics are marginal regressions of a
phenotype simulated from its genotypes."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import lassosum2_ref as ref  # noqa: E402

sparse = pytest.importorskip("scipy.sparse")


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def data(ba, golden_dir):
    gb = ba.bed(os.path.join(golden_dir, "example.bed"))
    G = ba.read_bed(gb, None, None).astype(np.float64)          # n x m, no missing values in this file
    keep = np.nonzero(G.std(axis=0) > 0)[0]
    G = G[:, keep]
    n, m = G.shape
    rng = np.random.default_rng(42)
    Z = (G - G.mean(axis=0)) / G.std(axis=0)
    b = np.where(rng.random(m) < 0.02, rng.normal(0, 0.3, m), 0.0)
    y = Z @ b + rng.normal(0, 1, n)
    # marginal least squares of y on each variant
    gc = G - G.mean(axis=0)
    yc = y - y.mean()
    sxx = (gc * gc).sum(axis=0)
    beta = gc.T @ yc / sxx
    resid = ((yc[:, None] - gc * beta) ** 2).sum(axis=0) / (n - 2)
    df = {"beta": beta, "beta_se": np.sqrt(resid / sxx),
          "n_eff": np.round(n * rng.uniform(0.8, 1.0, m))}
    return gb, keep, df


def _corr(ba, data, size):
    gb, keep, _ = data
    return ba.bed_cor(gb, ind_col=keep, size=size)


def _expected(corr, df, sub=None, **kw):
    """the restatement on the full columns of corr (upper triangle), scaled back as R/lassosum2.R:80 does"""
    from bigsnpr_amd.lassosum2 import _col_means_zero, lassosum2_inputs
    m2 = corr.Dim[1]
    fp, fi, fx = ref.full_from_upper(corr.p, corr.i, corr.x, m2)
    take = (lambda a: a) if sub is None else (lambda a: np.asarray(a)[sub])
    scale, bh, pf, lam, dl = lassosum2_inputs(take(df["beta"]), take(df["beta_se"]), take(df["n_eff"]),
                                              kw.pop("delta", (0.001, 0.01, 0.1, 1)), kw.pop("nlambda", 30),
                                              kw.pop("lambda_min_ratio", 0.01))
    beta, iters, moves, _ = ref.grid(fp, fi, fx, m2, bh, pf, lam, dl, ind_sub=sub, nthreads=16, **kw)
    return beta * scale[:, None], iters, _col_means_zero(beta)


def _same(res, exp):
    beta, iters, spars = exp
    assert res.shape == beta.shape
    assert np.array_equal(np.asarray(res), beta, equal_nan=True)
    gp = res.grid_param
    assert np.array_equal(gp["num_iter"], iters)
    assert np.array_equal(gp["sparsity"], spars, equal_nan=True)


def test_grid_equals_restatement_and_repeats(ba, data):
    corr = _corr(ba, data, 100)
    df = data[2]
    with ba.as_SFBM(corr) as sf:
        assert sf.ncol == corr.Dim[1] and sf.nnz == 2 * corr.x.size - corr.Dim[1]
        col = np.repeat(np.arange(corr.Dim[1]), np.diff(corr.p))
        assert sf.bandwidth == np.max(col - corr.i)
        res = ba.snp_lassosum2(sf, df, nlambda=10, maxiter=100)
        assert res.shape == (corr.Dim[1], 40)
        _same(res, _expected(corr, df, nlambda=10, maxiter=100))
        gp = res.grid_param
        assert np.all(gp["time"] > 0) and np.all(gp["num_iter"] <= 101)
        assert np.nanmax(gp["sparsity"]) > 0 and np.nanmin(gp["sparsity"]) < 1
        # deterministic: a second call gives the same bits (test-9-lassosum2.R)
        res2 = ba.snp_lassosum2(sf, df, nlambda=10, maxiter=100)
        assert np.array_equal(np.asarray(res2), np.asarray(res), equal_nan=True)
        assert np.array_equal(res2.grid_param["num_iter"], gp["num_iter"])


def test_subsets_via_ind_corr(ba, data):
    corr = _corr(ba, data, 100)
    df = data[2]
    m2 = corr.Dim[1]
    rng = np.random.default_rng(7)
    fp, fi, fx = ref.full_from_upper(corr.p, corr.i, corr.x, m2)
    full = sparse.csc_matrix((fx, fi, fp), shape=(m2, m2))
    with ba.as_SFBM(corr) as sf:
        for sub in (np.sort(rng.choice(m2, 1500, replace=False)), rng.choice(m2, 1500, replace=False)):
            dsub = {k: np.asarray(v)[sub] for k, v in df.items()}
            res = ba.snp_lassosum2(sf, dsub, ind_corr=sub, nlambda=10, maxiter=50)
            _same(res, _expected(corr, df, sub=sub, nlambda=10, maxiter=50))
            # lassosum2(corr[sub, sub]) == lassosum2(corr, ind.corr = sub), here bit for bit
            res_sub = ba.snp_lassosum2(full[sub][:, sub], dsub, nlambda=10, maxiter=50)
            assert np.array_equal(np.asarray(res_sub), np.asarray(res), equal_nan=True)
            assert np.array_equal(res_sub.grid_param["num_iter"], res.grid_param["num_iter"])


def test_every_input_form_gives_the_same_bits(ba, data):
    corr = _corr(ba, data, 60)
    df = data[2]
    m2 = corr.Dim[1]
    fp, fi, fx = ref.full_from_upper(corr.p, corr.i, corr.x, m2)
    forms = [corr,                                                        # CorResult (upper, expanded on the device)
             corr.tocsc(),                                                # scipy, upper triangle
             sparse.csc_matrix((fx, fi, fp), shape=(m2, m2)),             # scipy, full columns
             ba.SFBM(fp, fi, fx, m2, False),                              # full columns given directly
             ba.SFBM(corr.p, corr.i, corr.x, m2, True)]
    outs = [ba.snp_lassosum2(f, df, nlambda=5, delta=(0.01, 1), maxiter=30) for f in forms]
    for o in outs[1:]:
        assert np.array_equal(np.asarray(o), np.asarray(outs[0]), equal_nan=True)
        assert np.array_equal(o.grid_param["num_iter"], outs[0].grid_param["num_iter"])
    _same(outs[0], _expected(corr, df, nlambda=5, delta=(0.01, 1), maxiter=30))
    for f in forms[3:]:
        f.close()


def test_more_grid_points_than_compute_units(ba, data):
    gb, keep, df = data
    cols = keep[:600]
    corr = ba.bed_cor(gb, ind_col=cols, size=40)
    d = {k: np.asarray(v)[:600] for k, v in df.items()}
    res = ba.snp_lassosum2(corr, d, nlambda=80, maxiter=40)
    assert res.shape == (600, 320)
    _same(res, _expected(corr, d, nlambda=80, maxiter=40))


def test_divergence_and_dfmax_stop(ba, data):
    corr = _corr(ba, data, 500)     # a wide window of 517 samples: far from positive definite
    df = data[2]
    res = ba.snp_lassosum2(corr, df, nlambda=6, delta=(0.001, 1), maxiter=30)
    nan_cols = np.isnan(np.asarray(res)).all(axis=0)
    assert nan_cols.any() and not nan_cols.all()
    assert np.isnan(res.grid_param["sparsity"][nan_cols]).all()
    _same(res, _expected(corr, df, nlambda=6, delta=(0.001, 1), maxiter=30))
    res = ba.snp_lassosum2(corr, df, nlambda=6, delta=(1,), maxiter=30, dfmax=20)
    nz = (np.asarray(res) != 0).sum(axis=0)
    assert (nz > 20).any()                              # stopped on df > dfmax, not on convergence
    _same(res, _expected(corr, df, nlambda=6, delta=(1,), maxiter=30, dfmax=20))
