"""lassosum2 without a GPU: the C statement (tests/native/lassosum2_ref.c) against a line-by-line Python transliteration of
src/lassosum2.cpp, the grid snp_lassosum2 builds (R/lassosum2.R:49-57), the reference's argument errors and the host
checks of as_SFBM."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import lassosum2_ref as ref  # noqa: E402

sparse = pytest.importorskip("scipy.sparse")


def banded_corr(m2, band, seed, n=60):
    """a correlation matrix of random genotypes, entries beyond `band` dropped (not positive definite in general)"""
    rng = np.random.default_rng(seed)
    X = rng.binomial(2, rng.uniform(0.1, 0.5, m2), size=(n, m2)).astype(float)
    R = np.corrcoef(X, rowvar=False)
    R[np.isnan(R)] = 0
    jj, ii = np.meshgrid(np.arange(m2), np.arange(m2))
    R[np.abs(ii - jj) > band] = 0
    np.fill_diagonal(R, 1.0)
    return sparse.csc_matrix(R)


def chain_corr(m2, rho):
    """tridiagonal with rho off the diagonal: not positive definite for rho > 0.5 at large m2 (diverges)"""
    R = sparse.diags([np.full(m2 - 1, rho), np.ones(m2), np.full(m2 - 1, rho)], [-1, 0, 1])
    return sparse.csc_matrix(R)


def sumstats(A, seed, causal=0.2, N=2000):
    rng = np.random.default_rng(seed)
    m2 = A.shape[0]
    b = np.where(rng.random(m2) < causal, rng.normal(0, 0.2, m2), 0.0)
    return A @ b + rng.normal(0, 1 / np.sqrt(N), m2)


def _compare(A, bh, pf, lam, dl, sub=None, **kw):
    p, i, x = ref.full_csc(A)
    m2 = A.shape[0]
    beta, iters, moves, _ = ref.grid(p, i, x, m2, bh, pf, lam, dl, ind_sub=sub, nthreads=2, **kw)
    for g in range(lam.size):
        pb, pk = ref.py_one(p, i, x, m2, bh, pf * lam[g], pf * dl[g] + 1, sub, kw.get("dfmax", 200e3),
                            kw.get("maxiter", 1000), kw.get("tol", 1e-5))
        assert np.array_equal(beta[:, g], pb, equal_nan=True), g
        assert iters[g] == pk, (g, iters[g], pk)
    return beta, iters, moves


def test_c_statement_equals_python_transliteration():
    A = banded_corr(90, 6, seed=1)
    bh = sumstats(A, 2)
    pf = np.sqrt(1 / np.random.default_rng(3).uniform(0.5, 1, 90))
    lam0 = np.max(np.abs(bh / pf))
    lam = np.tile(lam0 * np.array([0.7, 0.2, 0.05, 0.01]), 2)
    dl = np.repeat([0.01, 1.0], 4)
    beta, iters, moves = _compare(A, bh, pf, lam, dl, maxiter=60)
    assert np.all(moves > 0) and np.all(iters >= 2)
    # a subset of the columns, unsorted, and a sorted one
    rng = np.random.default_rng(4)
    for sub in (rng.permutation(90)[:50], np.sort(rng.permutation(90)[:40])):
        _compare(A, bh[sub], pf[sub], lam[:3], dl[:3], sub=sub, maxiter=40)


def test_divergence_dfmax_and_maxiter_cases():
    A = chain_corr(60, 0.9)
    bh = sumstats(A, 5, causal=0.5)
    pf = np.ones(60)
    lam0 = np.max(np.abs(bh))
    # diverging: small lambda and delta on a matrix that is not positive definite
    beta, iters, _ = _compare(A, bh, pf, np.array([lam0 * 0.001, lam0 * 0.5]), np.array([0.001, 0.001]))
    assert np.isnan(beta[:, 0]).all() and not np.isnan(beta[:, 1]).any()
    # dfmax stop after the first sweep
    A = banded_corr(70, 4, seed=6)
    bh = sumstats(A, 7)
    beta, iters, _ = _compare(A, bh, np.ones(70), np.array([1e-4]), np.array([0.5]), dfmax=5)
    assert iters[0] == 1 and np.count_nonzero(beta[:, 0]) > 5
    # maxiter runs out: num_iter = maxiter + 1
    beta, iters, _ = _compare(A, bh, np.ones(70), np.array([1e-4]), np.array([0.01]), maxiter=3, tol=0.0)
    assert iters[0] == 4


def test_explicit_zeros_and_nan_propagate_like_the_loop():
    A = banded_corr(40, 3, seed=8).tolil()
    A[5, 7] = A[7, 5] = np.nan
    A = sparse.csc_matrix(A)
    bh = sumstats(sparse.csc_matrix(np.nan_to_num(A.toarray())), 9)
    _compare(A, bh, np.ones(40), np.array([0.01, 0.001]), np.array([0.1, 0.1]), maxiter=20)


def test_grid_inputs_follow_the_reference():
    import bigsnpr_amd as ba
    from bigsnpr_amd.lassosum2 import lassosum2_inputs
    beta = np.array([0.1, -0.3, 0.02, 0.0, 0.25])
    se = np.array([0.05, 0.1, 0.02, 0.04, 0.1])
    n = np.array([1000.0, 4000.0, 2000.0, 4000.0, 500.0])
    scale, bh, pf, lam, dl = lassosum2_inputs(beta, se, n, (0.001, 0.01, 0.1, 1), 30, 0.01)
    assert np.array_equal(scale, np.sqrt(n * (se * se) + beta * beta))
    assert np.array_equal(bh, beta / scale)
    assert np.array_equal(pf, np.sqrt(4000.0 / n))
    lambda0 = np.max(np.abs(bh / pf))
    seq = ba.seq_log(lambda0, 0.01 * lambda0, 31)[1:]
    assert lam.size == 120 and dl.size == 120
    assert np.array_equal(lam[:30], seq) and np.array_equal(lam[90:], seq)      # lambda varies fastest
    assert np.array_equal(dl, np.repeat([0.001, 0.01, 0.1, 1.0], 30))
    assert lam[0] < lambda0 and np.isclose(lam[29], 0.01 * lambda0)


def _df(m, seed=0):
    rng = np.random.default_rng(seed)
    return {"beta": rng.normal(0, 0.1, m), "beta_se": np.full(m, 0.05), "n_eff": np.full(m, 1000.0)}


def test_argument_errors_before_gpu_work():
    import bigsnpr_amd as ba
    A = banded_corr(20, 2, seed=1)
    df = _df(20)
    for drop, name in (("beta", "beta"), ("beta_se", "beta_se"), ("n_eff", "n_eff")):
        bad = {k: v for k, v in df.items() if k != drop}
        with pytest.raises(ValueError, match="'df_beta' should have element '%s'." % name):
            ba.snp_lassosum2(A, bad)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_lassosum2(A, _df(19))
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_lassosum2(A, _df(5), ind_corr=np.arange(4))
    with pytest.raises(ValueError, match="all\\(ind.corr %in% cols_along\\(corr\\)\\) is not TRUE"):
        ba.snp_lassosum2(A, _df(3), ind_corr=[0, 5, 20])
    bad = dict(df, beta_se=np.where(np.arange(20) == 3, 0.0, 0.05))
    with pytest.raises(ValueError, match="'df_beta\\$beta_se' should have only positive values."):
        ba.snp_lassosum2(A, bad)
    with pytest.raises(ValueError, match="'delta' should have only positive values."):
        ba.snp_lassosum2(A, df, delta=(0.1, 0))
    with pytest.raises(TypeError, match="'corr' should be"):
        ba.snp_lassosum2(np.eye(20), df)


def test_as_SFBM_host_checks():
    import bigsnpr_amd as ba
    from bigsnpr_amd.lassosum2 import SFBM
    with pytest.raises(ValueError, match="square"):
        ba.as_SFBM(sparse.csc_matrix(np.ones((3, 4))))
    with pytest.raises(TypeError):
        ba.as_SFBM(np.eye(3))
    p = np.array([0, 1, 3, 4])
    with pytest.raises(ValueError, match="ncol\\(corr\\) \\+ 1"):
        SFBM(p[:3], [0, 0, 1, 2], np.ones(4), 3, False)
    with pytest.raises(ba.BsnError, match="non-decreasing"):
        SFBM([0, 3, 1, 4], [0, 0, 1, 2], np.ones(4), 3, False)
    with pytest.raises(ba.BsnError, match="start at 0"):
        SFBM([1, 1, 3, 4], [0, 0, 1, 2], np.ones(4), 3, False)
    with pytest.raises(ba.BsnError, match="out of range"):
        SFBM(p, [0, 0, 3, 2], np.ones(4), 3, False)
    with pytest.raises(ba.BsnError, match="strictly increasing"):
        SFBM(p, [0, 1, 0, 2], np.ones(4), 3, False)
    with pytest.raises(ba.BsnError, match="strictly increasing"):
        SFBM(p, [0, 1, 1, 2], np.ones(4), 3, False)
    with pytest.raises(ba.BsnError, match="upper-triangular"):
        SFBM([0, 2, 3, 4], [0, 1, 1, 2], np.ones(4), 3, True)
    if ba.device_count() == 0:
        # a valid matrix gets past the host checks and then needs the device
        with pytest.raises(ba.BsnError, match="no CPU fallback"):
            SFBM(p, [0, 0, 1, 2], np.ones(4), 3, True)
