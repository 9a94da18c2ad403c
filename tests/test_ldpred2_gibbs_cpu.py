"""LDpred2-grid's Gibbs sampler without a GPU: the shared header bigsnpr_amd/csrc/gibbs_step.hpp built with g++ (generator,
exp / log / inverse normal CDF), the C statement (tests/native/ldpred2_ref.cpp) against a line-by-line Python
transliteration of src/ldpred2.cpp and src/ldpred2-sampling.cpp, what the chains converge to, and the argument checks
of snp_ldpred2_grid."""
import math
import os
import statistics
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ldpred2_ref as ref  # noqa: E402
from sfbm_inputs import banded_corr  # noqa: E402
from scipy import sparse  # noqa: E402


# ---- the shared header ------------------------------------------------------------------------------------------------------

def test_philox_known_answers_and_python_transliteration():
    # the known-answer vectors of Random123 for philox4x32-10
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert tuple(ref.philox(ctr, key)) == out
        assert tuple(ref.py_philox(ctr, key)) == out
    rng = np.random.default_rng(1)
    for _ in range(3000):
        ctr, key = rng.integers(0, 2 ** 32, 4), rng.integers(0, 2 ** 32, 2)
        assert ref.philox(ctr, key) == ref.py_philox(ctr, key)


def test_draws_equal_the_transliteration_and_depend_on_the_counter_alone():
    seed, stream = 0x123456789abcdef0, (7 << 32) | 5
    U, Z = ref.draws(seed, stream, 3, 500)
    pU, pV = ref.py_draws(seed, stream, 3, 500)
    assert np.array_equal(U, pU)
    assert np.array_equal(Z, ref.qnorm_det(pV))
    # position j alone, not where the batch starts
    U2, Z2 = ref.draws(seed, stream, 3, 100, j0=400)
    assert np.array_equal(U2, U[400:]) and np.array_equal(Z2, Z[400:])
    for other in (ref.draws(seed + 1, stream, 3, 500), ref.draws(seed, stream + 1, 3, 500), ref.draws(seed, stream, 4, 500)):
        assert not np.any(other[0] == U)


def test_uniform_and_normal_moments():
    """1e6 draws: mean and variance within 5 standard errors of 1/2, 1/12, 0 and 1.  The standard errors follow from n:
    sd(U) / sqrt(n), sqrt((E(U - 1/2)^4 - 1/144) / n) = sqrt(1 / 180 n), 1 / sqrt(n) and sqrt(2 / n)."""
    n = 1000000
    U, Z = ref.draws(2024, 11, 0, n)
    assert U.min() > 0 and U.max() < 1
    assert np.all(U * 2.0 ** 53 % 2 == 1)           # odd 53-bit numerators: exact, symmetric about 1/2
    assert abs(U.mean() - 0.5) < 5 * math.sqrt(1 / 12 / n)
    assert abs(U.var() - 1 / 12) < 5 * math.sqrt(1 / 180 / n)
    assert abs(Z.mean()) < 5 / math.sqrt(n)
    assert abs(Z.var() - 1) < 5 * math.sqrt(2 / n)
    assert abs(np.corrcoef(U, Z)[0, 1]) < 5 / math.sqrt(n)
    assert np.all(np.isfinite(Z)) and np.abs(Z).max() < 8.3      # the inverse CDF of 2^-53 is -8.21


def test_exp_log_qnorm_against_libm():
    """within 1e-13 relative on the ranges the sampler uses: exp of -C3^2 / C4 / 2 <= 0 (0 below -708, where the true value
    is below 3.4e-308), log of a uniform's smaller tail (2^-53, 0.075], the inverse CDF of a uniform in [2^-53, 1 - 2^-53]"""
    x = np.concatenate([np.linspace(-708, 0, 200001), -np.exp(np.linspace(-40, 6.5, 20001)), [0.0, -0.0]])
    assert np.max(np.abs(ref.exp_det(x) / np.exp(x) - 1)) <= 1e-13
    assert np.array_equal(ref.exp_det([-709.0, -1e300, -np.inf]), [0, 0, 0])
    assert np.isnan(ref.exp_det([np.nan])[0]) and ref.exp_det([np.inf])[0] == np.inf
    x = np.concatenate([np.exp(np.linspace(math.log(2.0 ** -53), math.log(0.075), 100001)), np.linspace(0.075, 0.5, 1001)])
    assert np.max(np.abs(ref.log_det(x) / np.log(x) - 1)) <= 1e-13
    nd = statistics.NormalDist()
    rng = np.random.default_rng(0)
    tails = 2.0 ** -53 * np.arange(1, 4000, 2)
    u = np.concatenate([rng.random(100000), tails, 1 - tails, np.linspace(0.07, 0.08, 1001), np.linspace(0.92, 0.93, 1001),
                        np.exp(np.linspace(math.log(2.0 ** -53), math.log(0.5), 20001))])
    u = u[u != 0.5]
    want = np.array([nd.inv_cdf(v) for v in u])
    assert np.max(np.abs(ref.qnorm_det(u) - want) / np.abs(want)) <= 1e-13
    assert ref.qnorm_det([0.5])[0] == 0


# ---- the C statement against the transliteration -------------------------------------------------------------------------------

def sumstats(A, seed, causal=0.2, N=2000):
    rng = np.random.default_rng(seed)
    m2 = A.shape[0]
    b = np.where(rng.random(m2) < causal, rng.normal(0, 0.2, m2), 0.0)
    return A @ b + rng.normal(0, 1 / np.sqrt(N), m2)


def _uz(seed, stream, sweeps, m):
    UZ = [ref.draws(seed, stream, k, m) for k in range(sweeps)]
    return [u for u, _ in UZ], [z for _, z in UZ]


@pytest.mark.parametrize("sub_kind", ["all", "sorted", "shuffled"])
def test_c_statement_equals_python_transliteration(sub_kind):
    m2 = 80
    A = banded_corr(m2, 6, seed=1)
    p, i, x = ref.full_csc(A)
    rng = np.random.default_rng(4)
    sub = {"all": None, "sorted": np.sort(rng.permutation(m2)[:45]), "shuffled": rng.permutation(m2)[:50]}[sub_kind]
    bh = sumstats(A, 2)
    nv = np.round(rng.uniform(1500, 2000, m2))
    if sub is not None:
        bh, nv = bh[sub], nv[sub]
    m = bh.size
    burn, it, seed = 5, 12, 99
    h2 = np.array([0.3, 0.3, 0.1, 0.5])
    pp = np.array([1.0, 0.1, 0.01, 0.3])
    for sp in (0, 1):
        beta, moves, _ = ref.grid(p, i, x, m2, bh, nv, h2, pp, np.full(4, sp), ind_sub=sub, stream=[0, 1, 2, 9],
                                  burn_in=burn, num_iter=it, seed=seed, nthreads=2)
        assert np.all(moves > 0)
        for g, st in enumerate([0, 1, 2, 9]):
            U, Z = _uz(seed, st, burn + it, m)
            want = ref.py_gibbs_one(p, i, x, m2, bh, nv, sub, h2[g], pp[g], bool(sp), burn, it, U, Z)
            assert np.array_equal(beta[:, g], want, equal_nan=True), (sp, g)
            smp, _ = ref.sampling(p, i, x, m2, bh, nv, h2[g], pp[g], sp, ind_sub=sub, stream=st, burn_in=burn, num_iter=it,
                                  seed=seed)
            want = ref.py_gibbs_one_sampling(p, i, x, m2, bh, nv, sub, h2[g], pp[g], bool(sp), burn, it, U, Z)
            assert np.array_equal(smp, want), (sp, g)
        if sp:
            assert np.mean(beta[:, 2] == 0) > 0.3          # the sparse branch is exercised
    # the thread count changes nothing
    b1, _, _ = ref.grid(p, i, x, m2, bh, nv, h2, pp, np.zeros(4), ind_sub=sub, burn_in=burn, num_iter=it, seed=seed, nthreads=1)
    b4, _, _ = ref.grid(p, i, x, m2, bh, nv, h2, pp, np.zeros(4), ind_sub=sub, burn_in=burn, num_iter=it, seed=seed, nthreads=4)
    assert np.array_equal(b1, b4)


def test_statement_diverges_like_the_transliteration():
    """a matrix that is not positive definite and an inflated h2: the NaN column of the reference's divergence stop"""
    m2 = 60
    A = sparse.csc_matrix(sparse.diags([np.full(m2 - 1, 0.9), np.ones(m2), np.full(m2 - 1, 0.9)], [-1, 0, 1]))
    p, i, x = ref.full_csc(A)
    bh = sumstats(A, 5, causal=0.5)
    nv = np.full(m2, 2000.0)
    h2, pp = np.array([50.0, 0.001]), np.array([1.0, 1.0])
    beta, _, _ = ref.grid(p, i, x, m2, bh, nv, h2, pp, np.zeros(2), burn_in=10, num_iter=10, seed=3)
    assert np.isnan(beta[:, 0]).all() and np.isfinite(beta[:, 1]).all()
    U, Z = _uz(3, 0, 20, m2)
    assert np.isnan(ref.py_gibbs_one(p, i, x, m2, bh, nv, None, 50.0, 1.0, False, 10, 10, U, Z)).all()


def test_subset_equals_the_submatrix():
    """ldpred2(corr, ind.corr = sub) == ldpred2(corr[sub, sub]) (test-8-LDpred2.R:266-287): the counter uses the position
    in the subset, and the rows outside it are never read"""
    m2 = 120
    A = banded_corr(m2, 8, seed=11)
    rng = np.random.default_rng(12)
    for sub in (np.sort(rng.permutation(m2)[:70]), rng.permutation(m2)[:70]):
        bh, nv = sumstats(A, 13)[sub], np.full(70, 1800.0)
        h2, pp, sp = np.array([0.3, 0.3]), np.array([0.05, 1.0]), np.array([1, 0])
        full, _, _ = ref.grid(*ref.full_csc(A), m2, bh, nv, h2, pp, sp, ind_sub=sub, burn_in=8, num_iter=10, seed=5)
        part, _, _ = ref.grid(*ref.full_csc(A[sub][:, sub]), 70, bh, nv, h2, pp, sp, burn_in=8, num_iter=10, seed=5)
        assert np.array_equal(full, part)


def test_window_rule():
    """the host rule of the LDS window: ascending order and an envelope within the budget"""
    m2 = 700
    A = banded_corr(m2, 30, seed=21)
    p, i, x = ref.full_csc(A)
    fits, rows = ref.envelope(p, i, m2)
    # rows lo[b] .. hi[b] of a band of half-width 30 and 64 positions per block
    assert fits and rows == 64 + 2 * 30
    fits, rows = ref.envelope(p, i, m2, np.arange(0, m2, 2))
    assert fits and rows == 2 * 63 + 1 + 2 * 30
    fits, rows = ref.envelope(p, i, m2, np.arange(m2)[::-1])
    assert not fits
    # a few far entries per column: the envelope, not the count of entries, decides
    W = ref.window_rows()
    for half, want in ((W // 2 - 40, True), (W // 2, False)):
        m2 = 20000
        d = np.arange(m2 - half)
        B = sparse.coo_matrix((np.full(d.size, 0.01), (d, d + half)), shape=(m2, m2))
        B = sparse.csc_matrix(B + B.T + sparse.identity(m2))
        p, i, x = ref.full_csc(B)
        fits, rows = ref.envelope(p, i, m2)
        assert fits == want and rows == 2 * half + 64, (half, rows)


# ---- what the chains converge to ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def example(golden_dir):
    """tests/test_gpu_lassosum2.py's fixture on the host: example.bed, the same simulated phenotype and marginal
    regressions, and the dense correlation windowed to |i - j| <= 100"""
    raw = np.fromfile(os.path.join(golden_dir, "example.bed"), dtype=np.uint8)
    n = sum(1 for _ in open(os.path.join(golden_dir, "example.fam")))
    mm = sum(1 for _ in open(os.path.join(golden_dir, "example.bim")))
    pitch = (n + 3) // 4
    by = raw[3:].reshape(mm, pitch)
    codes = np.stack([(by >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(mm, pitch * 4)[:, :n]
    assert not np.any(codes == 1)                               # no missing value in this file
    G = np.array([2.0, np.nan, 1.0, 0.0])[codes].T               # n x m: 00 -> 2, 10 -> 1, 11 -> 0
    keep = np.nonzero(G.std(axis=0) > 0)[0]
    G = G[:, keep]
    n, m = G.shape
    rng = np.random.default_rng(42)
    Z = (G - G.mean(axis=0)) / G.std(axis=0)
    b = np.where(rng.random(m) < 0.02, rng.normal(0, 0.3, m), 0.0)
    y = Z @ b + rng.normal(0, 1, n)
    gc = G - G.mean(axis=0)
    yc = y - y.mean()
    sxx = (gc * gc).sum(axis=0)
    beta = gc.T @ yc / sxx
    resid = ((yc[:, None] - gc * beta) ** 2).sum(axis=0) / (n - 2)
    df = {"beta": beta, "beta_se": np.sqrt(resid / sxx), "n_eff": np.round(n * rng.uniform(0.8, 1.0, m))}
    R = (Z.T @ Z) / n
    ii, jj = np.nonzero(np.abs(np.subtract.outer(np.arange(m), np.arange(m))) <= 100)
    A = sparse.csc_matrix((R[ii, jj], (ii, jj)), shape=(m, m))
    scale = np.sqrt(df["n_eff"] * df["beta_se"] ** 2 + df["beta"] ** 2)
    return A, df["beta"] / scale, df["n_eff"]


def test_p_one_converges_to_the_infinitesimal_posterior_mean(example):
    """p = 1, non-sparse: post_p = 1, and the average tends to (R + diag(m / (h2 N)))^-1 beta_hat, snp_ldpred2_inf before
    scaling.  The reference loop with numpy's generator on this input measured ||grid - inf|| / ||inf|| = 0.0108 - 0.0110
    at num_iter 100 and 0.0052 - 0.0055 at 400 over three seeds each (seed-to-seed spread 3 %); the bound at 100 is twice
    that figure, 0.022.  A wrong constant or a stale dotprods gives an error of order 1."""
    A, bh, nv = example
    m = bh.size
    h2 = 0.3
    inf = np.linalg.solve(A.toarray() + np.diag(m / (h2 * nv)), bh)
    p, i, x = ref.full_csc(A)
    errs = {}
    for it in (100, 400):
        beta, _, _ = ref.grid(p, i, x, m, bh, nv, [h2], [1.0], [0], burn_in=50, num_iter=it, seed=20240 + it, nthreads=1)
        assert np.isfinite(beta).all()
        errs[it] = np.linalg.norm(beta[:, 0] - inf) / np.linalg.norm(inf)
        print("num_iter %d: ||grid - inf|| / ||inf|| = %.4f, cor %.6f" % (it, errs[it], np.corrcoef(beta[:, 0], inf)[0, 1]))
    assert errs[100] <= 0.022
    assert errs[400] < errs[100]


def test_sparse_chains_and_sampling_betas(example):
    """p = 0.01 (test-8-LDpred2.R:51-66): the mean of the sampling betas (num_iter 200) follows the grid column, cor > 0.9
    (the reference's own assertion; its loop with numpy's generator measured 0.998 here); the non-sparse column has no
    exact zero; more than half of the sparse column is exactly zero (measured 0.67); no column is NaN, although the
    matrix's smallest eigenvalue is -0.50"""
    A, bh, nv = example
    m = bh.size
    p, i, x = ref.full_csc(A)
    beta, _, _ = ref.grid(p, i, x, m, bh, nv, [0.3, 0.3], [0.01, 0.01], [0, 1], burn_in=50, num_iter=100, seed=77, nthreads=2)
    assert np.isfinite(beta).all()
    smp, _ = ref.sampling(p, i, x, m, bh, nv, 0.3, 0.01, 0, stream=5, burn_in=50, num_iter=200, seed=78)
    assert smp.shape == (m, 200)
    cor = np.corrcoef(smp.mean(axis=1), beta[:, 0])[0, 1]
    zeros = np.mean(beta[:, 1] == 0)
    print("cor(rowMeans(sampling), grid) = %.4f, exact zeros in the sparse column = %.3f" % (cor, zeros))
    assert cor > 0.9
    assert not np.any(beta[:, 0] == 0)
    assert zeros > 0.5


# ---- the wrapper's checks ------------------------------------------------------------------------------------------------------

def _df(m, seed=0):
    rng = np.random.default_rng(seed)
    return {"beta": rng.normal(0, 0.1, m), "beta_se": np.full(m, 0.05), "n_eff": np.full(m, 1000.0)}


def test_argument_errors_before_gpu_work():
    import bigsnpr_amd as ba
    A = banded_corr(20, 2, seed=1)
    df = _df(20)
    gp = {"p": [0.1, 1.0], "h2": [0.3, 0.3], "sparse": [False, True]}
    for name in ("beta", "beta_se", "n_eff"):
        bad = {k: v for k, v in df.items() if k != name}
        with pytest.raises(ValueError, match="'df_beta' should have element '%s'." % name):
            ba.snp_ldpred2_grid(A, bad, gp)
    for name in ("p", "h2", "sparse"):
        bad = {k: v for k, v in gp.items() if k != name}
        with pytest.raises(ValueError, match="'grid_param' should have element '%s'." % name):
            ba.snp_ldpred2_grid(A, df, bad)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldpred2_grid(A, _df(19), gp)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldpred2_grid(A, _df(5), gp, ind_corr=np.arange(4))
    with pytest.raises(ValueError, match="all\\(ind.corr %in% cols_along\\(corr\\)\\) is not TRUE"):
        ba.snp_ldpred2_grid(A, _df(3), gp, ind_corr=[0, 5, 20])
    bad = dict(df, beta_se=np.where(np.arange(20) == 3, 0.0, 0.05))
    with pytest.raises(ValueError, match="'df_beta\\$beta_se' should have only positive values."):
        ba.snp_ldpred2_grid(A, bad, gp)
    with pytest.raises(ValueError, match="'grid_param\\$h2' should have only positive values."):
        ba.snp_ldpred2_grid(A, df, dict(gp, h2=[0.3, 0.0]))
    with pytest.raises(ValueError, match="'ncores' should be an integer >= 1."):
        ba.snp_ldpred2_grid(A, df, gp, ncores=0)
    with pytest.raises(ValueError, match="Only one set of parameters is allowed when using 'return_sampling_betas'."):
        ba.snp_ldpred2_grid(A, df, gp, return_sampling_betas=True)
    with pytest.raises(ValueError, match="repeated"):
        ba.snp_ldpred2_grid(A, _df(3), gp, ind_corr=[1, 4, 1])
    with pytest.raises(ValueError, match="'num_iter' should be at least 1."):
        ba.snp_ldpred2_grid(A, df, gp, num_iter=0)
    with pytest.raises(ValueError, match="'burn_in' should not be negative."):
        ba.snp_ldpred2_grid(A, df, gp, burn_in=-1)
    with pytest.raises(TypeError, match="'corr' should be"):
        ba.snp_ldpred2_grid(np.eye(20), df, gp)
    if ba.device_count() == 0:
        # everything valid gets past the host checks and then needs the device
        with pytest.raises(ba.BsnError, match="no CPU fallback"):
            ba.snp_ldpred2_grid(A, df, gp)
