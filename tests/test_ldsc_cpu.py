"""LD score regression (R/ldsc.R) and the argument checks of the LDSC / LDpred2-inf entry points, without a GPU: snp_ldsc is
numpy on the host; everything checked of snp_ldsc2, snp_ldpred2_inf, sp_prodVec and sp_solve_sym here is raised before any
device work."""
import math

import numpy as np
import pytest

import bigsnpr_amd as ba
from bigsnpr_amd import ldpred2

sparse = pytest.importorskip("scipy.sparse")


def planted(n_const, seed=1, M=5000, a=1.05, h2=0.3):
    rng = np.random.default_rng(seed)
    ld = rng.gamma(2, 20, M) + 1
    N = np.full(M, 50000.0) if n_const else rng.uniform(2e4, 8e4, M)
    return ld, N, a + h2 * N * ld / M - 1e-8, a, h2


@pytest.mark.parametrize("n_const", [True, False])
def test_planted_line_is_recovered_to_rounding(n_const):
    """chi2 = a + h2 N ld / M - 1e-8: the fit is exact, so the first reweighting round already has a zero residual, in
    step 1 (the values below chi2_thr1 = 30, a proper subset) and in step 2 (all of them).  Only the rounding of a 2 x 2
    normal equation is involved: a transliteration of R/ldsc.R:85-122 recovers both within 4e-15 relative on these data;
    1e-12 leaves three orders for another summation order in another numpy build."""
    ld, N, chi2, a, h2 = planted(n_const)
    below = int(np.sum(chi2 + 1e-8 < 30))
    assert 200 < below < ld.size - 200          # many values on each side of the threshold
    res = ba.snp_ldsc(ld, ld.size, chi2, N[0] if n_const else N, blocks=None)
    assert list(res) == ["int", "h2"]
    print("below the threshold: %d, int rel. error %.2e, h2 rel. error %.2e" % (below, abs(res["int"] / a - 1), abs(res["h2"] / h2 - 1)))
    assert abs(res["int"] / a - 1) <= 1e-12
    assert abs(res["h2"] / h2 - 1) <= 1e-12


def test_one_reweighting_step_equals_weighted_least_squares():
    rng = np.random.default_rng(2)
    n = 400
    x, y, w = rng.uniform(0, 50, n), rng.uniform(0.5, 40, n), rng.uniform(0.01, 2, n)
    sw = np.sqrt(w)
    # with an intercept: lm.wfit(cbind(1, x), y, w)
    coef = np.linalg.lstsq(np.column_stack([sw, sw * x]), sw * y, rcond=None)[0]
    alpha, beta, pred = ldpred2.wlm(x, y, w)
    assert np.allclose([alpha, beta], coef, rtol=1e-10, atol=0)
    assert np.allclose(pred, coef[0] + coef[1] * x, rtol=1e-10, atol=0)
    # without: lm.wfit(as.matrix(x), y, w)
    coef = np.linalg.lstsq((sw * x)[:, None], sw * y, rcond=None)[0]
    beta, pred = ldpred2.wlm_no_int(x, y, w)
    assert np.allclose(beta, coef[0], rtol=1e-10, atol=0) and np.allclose(pred, coef[0] * x, rtol=1e-10, atol=0)
    # the weights of R/ldsc.R:4-6
    assert np.array_equal(ldpred2.WEIGHTS(y, w), 1 / (y ** 2 * w))


def noisy(seed, M=600):
    rng = np.random.default_rng(seed)
    ld = rng.gamma(2, 20, M) + 1
    N = rng.uniform(2e4, 8e4, M)
    chi2 = (1.1 + 0.25 * N * ld / M) * rng.chisquare(1, M)
    return ld, N, chi2


def brute_jackknife(ld, M_size, chi2, N, blocks, **kw):
    """delete-a-group jackknife (https://doi.org/10.1023/A:1008800423698) written out: one fit without each block, then
    the pseudo-values.  The reference's inner calls see the chi2 it has already shifted by 1e-8 (R/ldsc.R:73, :140)."""
    M = chi2.size
    chi2 = chi2 + 1e-8
    ids = sorted(set(blocks.tolist()))
    full = ba.snp_ldsc(ld, M_size, chi2, N, blocks=None, **kw)
    ints, h2s, hs = [], [], []
    for g in ids:
        keep = [k for k in range(M) if blocks[k] != g]
        r = ba.snp_ldsc(ld[keep], M_size, chi2[keep], N[keep], blocks=None, **kw)
        ints.append(r["int"])
        h2s.append(r["h2"])
        hs.append(M / (M - len(keep)))
    out = {}
    for name, est, dels in (("int", full["int"], ints), ("h2", full["h2"], h2s)):
        pseudo = [h * est - (h - 1) * d for h, d in zip(hs, dels)]
        J = sum(p / h for p, h in zip(pseudo, hs))
        out[name] = J
        out[name + "_se"] = math.sqrt(sum((p - J) ** 2 / (h - 1) for p, h in zip(pseudo, hs)) / len(hs))
    return out


def test_jackknife_equals_its_definition():
    ld, N, chi2 = noisy(3)
    M = chi2.size
    # a number of blocks: sort(rep_len(seq_len(blocks), M))
    res = ba.snp_ldsc(ld, M, chi2, N, blocks=7)
    assert list(res) == ["int", "int_se", "h2", "h2_se"]
    blocks = np.sort(np.array([(k % 7) + 1 for k in range(M)]))
    exp = brute_jackknife(ld, M, chi2, N, blocks)
    for k in exp:
        assert res[k] == pytest.approx(exp[k], rel=1e-10), k
    assert res["int_se"] > 0 and res["h2_se"] > 0
    # a block vector given explicitly (unequal blocks, labels in no order)
    blocks = np.random.default_rng(4).choice([3, 10, 11, 40, 41], M, p=[0.1, 0.2, 0.3, 0.15, 0.25])
    res = ba.snp_ldsc(ld, M, chi2, N, blocks=blocks)
    exp = brute_jackknife(ld, M, chi2, N, blocks)
    for k in exp:
        assert res[k] == pytest.approx(exp[k], rel=1e-10), k
    # blocks = None: two values
    assert list(ba.snp_ldsc(ld, M, chi2, N, blocks=None)) == ["int", "h2"]
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldsc(ld, M, chi2, N, blocks=blocks[:-1])


def test_fixed_intercept():
    ld, N, chi2 = noisy(5)
    # 8 blocks of 75: h_blocks = 8, so the pseudo-values h - (h - 1) and their sum over 1 / h are exact in binary
    res = ba.snp_ldsc(ld, ld.size, chi2, N, blocks=8, intercept=1)
    assert res["int"] == 1 and res["int_se"] == 0
    assert res["h2_se"] > 0
    res0 = ba.snp_ldsc(ld, ld.size, chi2, N, blocks=None, intercept=1)
    assert res0["int"] == 1
    assert res0["h2"] != ba.snp_ldsc(ld, ld.size, chi2, N, blocks=None)["h2"]


def test_chi2_thresholds_select_subsets():
    ld, N, chi2 = noisy(6, M=3000)
    M = chi2.size
    assert np.sum(chi2 + 1e-8 >= 30) > 20 and np.sum(chi2 + 1e-8 >= 80) > 3
    # both thresholds at 25: the same call on pre-filtered vectors
    keep = chi2 + 1e-8 < 25
    a = ba.snp_ldsc(ld, M, chi2, N, blocks=None, chi2_thr1=25, chi2_thr2=25)
    e = ba.snp_ldsc(ld[keep], M, chi2[keep], N[keep], blocks=None, chi2_thr1=np.inf, chi2_thr2=np.inf)
    assert a == e
    # chi2_thr1 alone: step 1 on the subset gives the intercept, step 2 runs on everything with that intercept
    keep = chi2 + 1e-8 < 30
    a = ba.snp_ldsc(ld, M, chi2, N, blocks=None, chi2_thr1=30)
    step1 = ba.snp_ldsc(ld[keep], M, chi2[keep], N[keep], blocks=None, chi2_thr1=np.inf)
    assert a["int"] == step1["int"]
    e = ba.snp_ldsc(ld, M, chi2, N, blocks=None, intercept=step1["int"])
    assert a == e
    assert a["h2"] != ba.snp_ldsc(ld, M, chi2, N, blocks=None, chi2_thr1=np.inf)["h2"]


def test_snp_ldsc_argument_checks():
    ld, N, chi2 = noisy(7, M=50)
    with pytest.raises(ValueError, match="'chi2' should have only positive values."):
        ba.snp_ldsc(ld, 50, -chi2, N)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldsc(ld[:-1], 50, chi2, N)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldsc(ld, 50, chi2, N[:-1])
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldsc(ld, [50, 50], chi2, N)
    with pytest.raises(ValueError, match="'ld_size' should contain only integers."):
        ba.snp_ldsc(ld, 50.5, chi2, N)


def test_coef_to_liab():
    # K_pop = 0.5: z = dnorm(0) = 1 / sqrt(2 pi), so (0.25 sqrt(2 pi))^2 / 0.25 = pi / 2
    assert ba.coef_to_liab(0.5) == pytest.approx(math.pi / 2, rel=1e-14)
    assert ba.coef_to_liab(0.5, K_gwas=0.2) == pytest.approx(math.pi / 8 / 0.16, rel=1e-14)
    for K in (0.01, 0.02, 0.2, 0.37):
        assert ba.coef_to_liab(K) == pytest.approx(ba.coef_to_liab(1 - K), rel=1e-14)
        assert ba.coef_to_liab(K, 0.3) == pytest.approx(ba.coef_to_liab(1 - K, 0.7), rel=1e-14)
    assert ba.coef_to_liab(0.02) == pytest.approx((0.02 * 0.98 / 0.04841814) ** 2 / 0.25, rel=1e-6)   # dnorm(qnorm(0.02))


def corr_and_df(m2=30):
    R = sparse.diags([np.full(m2 - 1, 0.3), np.ones(m2), np.full(m2 - 1, 0.3)], [-1, 0, 1], format="csc")
    rng = np.random.default_rng(8)
    return R, {"beta": rng.normal(0, 0.1, m2), "beta_se": rng.uniform(0.01, 0.02, m2), "n_eff": np.full(m2, 1000.0)}


def test_errors_before_any_device_work():
    """none of these reaches as_SFBM (which would fail for another reason on a machine without a GPU)"""
    R, df = corr_and_df()
    m2 = R.shape[0]
    # test-8-LDpred2.R:120: a missing column
    no_beta = {k: v for k, v in df.items() if k != "beta"}
    with pytest.raises(ValueError, match="'df_beta' should have element 'beta'."):
        ba.snp_ldpred2_inf(R, no_beta, 0.3)
    with pytest.raises(ValueError, match="'df_beta' should have element 'beta'."):
        ba.snp_ldsc2(R, no_beta)
    with pytest.raises(ValueError, match="'df_beta' should have element 'n_eff'."):
        ba.snp_ldsc2(R, {k: v for k, v in df.items() if k != "n_eff"})
    # wrong lengths
    short = {k: v[:-1] for k, v in df.items()}
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldpred2_inf(R, short, 0.3)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldsc2(R, short)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldsc2(R, df, ind_beta=np.arange(m2 - 1))
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.snp_ldsc2(R, dict(df, beta_se=df["beta_se"][:-1]))
    with pytest.raises(ValueError, match=r"all\(ind.beta %in% cols_along\(corr\)\) is not TRUE"):
        ba.snp_ldsc2(R, df, ind_beta=np.arange(1, m2 + 1))
    # beta_se <= 0, h2 <= 0
    bad = dict(df, beta_se=np.where(np.arange(m2) == 3, 0.0, df["beta_se"]))
    with pytest.raises(ValueError, match=r"'df_beta\$beta_se' should have only positive values."):
        ba.snp_ldpred2_inf(R, bad, 0.3)
    with pytest.raises(ValueError, match=r"'df_beta\$beta_se' should have only positive values."):
        ba.snp_ldsc2(R, bad)
    for h2 in (0, -0.1):
        with pytest.raises(ValueError, match="'h2' should have only positive values."):
            ba.snp_ldpred2_inf(R, df, h2)
    # a repeated index is refused by the product and by the solve; so are a wrong length and an index out of range
    x = np.ones(4)
    for f in (ba.sp_prodVec, ba.sp_cprodVec, ba.sp_solve_sym):
        with pytest.raises(ValueError, match="'ind.corr' should not have repeated indices."):
            f(R, x, ind_corr=[1, 5, 1, 7])
        with pytest.raises(ValueError, match="Incompatibility between dimensions"):
            f(R, x, ind_corr=[1, 5, 7])
        with pytest.raises(ValueError, match="Incompatibility between dimensions"):
            f(R, x)
        with pytest.raises(ValueError, match=r"all\(ind.corr %in% cols_along\(corr\)\) is not TRUE"):
            f(R, x, ind_corr=[1, 5, m2, 7])
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.sp_solve_sym(R, np.ones(m2), add_to_diag=np.ones(m2 - 1))
    with pytest.raises(ValueError, match="'tol' should have only positive values."):
        ba.sp_solve_sym(R, np.ones(m2), tol=0)
    with pytest.raises(ValueError, match=r"all\(ind_sub %in% cols_along\(corr\)\) is not TRUE"):
        ba.ld_scores_sfbm(R, [0, m2])
    with pytest.raises(TypeError, match="'corr' should be a CorResult, a scipy sparse matrix or an SFBM."):
        ba.sp_prodVec(object(), x)


def test_library_refuses_before_any_device_work():
    """the C entry points make the same checks themselves (a NULL handle, then the arguments), ahead of the first HIP call"""
    import ctypes as C
    L = ba.load()
    y = np.zeros(3)
    for rc in (L.bsn_sfbm_prodvec(None, y.ctypes.data_as(C.POINTER(C.c_double)), None, 3, y.ctypes.data_as(C.POINTER(C.c_double))),
               L.bsn_sfbm_ld_scores(None, None, 3, y.ctypes.data_as(C.POINTER(C.c_double))),
               L.bsn_sfbm_solve_sym(None, None, None, None, 3, 1e-10, 10, None, None, None)):
        assert rc != 0 and b"NULL 'corr'" in L.bsn_last_error()
