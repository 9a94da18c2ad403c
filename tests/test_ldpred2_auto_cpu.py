"""LDpred2-auto without a GPU: the shared header bigsnpr_amd/csrc/gibbs_auto.hpp built with g++ — the C statement
(tests/native/ldpred2_auto_ref.cpp) against a Python restatement of src/ldpred2-auto.cpp, the bounded MLE against
L-BFGS-B and a grid of its box, rbeta's moments, the bootstrap's index, the counters of the epilogue — and the argument
checks of snp_ldpred2_auto, which come before any device work."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ldpred2_auto_ref as ref  # noqa: E402
import ldpred2_ref as grid_ref  # noqa: E402
from sfbm_inputs import banded_corr  # noqa: E402
from scipy import optimize  # noqa: E402


# ---- the C statement against the restatement -------------------------------------------------------------------------------

@pytest.mark.parametrize("use_mle", [True, False])
def test_c_statement_equals_python_restatement(use_mle):
    m2, burn, it, step, seed = 150, 3, 4, 2, 77
    A = banded_corr(m2, 6, seed=1)
    p, i, x = ref.full_csc(A)
    rng = np.random.default_rng(4)
    b = np.where(rng.random(m2) < 0.2, rng.normal(0, 0.2, m2), 0.0)
    bh = A @ b + rng.normal(0, 1 / np.sqrt(2000), m2)
    nv = np.round(rng.uniform(1500, 2000, m2))
    lv = 2 * np.log(rng.uniform(0.5, 3.0, m2))
    p_inits, streams = [0.3, 0.01], [0, 5]
    p_bounds, a_bounds, mean_ld, shrink = (1e-5, 1.0), (-1.5, 0.5), 3.7, 0.9
    got = ref.auto(p, i, x, m2, bh, nv, lv, p_inits, 0.3, mean_ld, stream=streams, burn_in=burn, num_iter=it, report_step=step,
                   no_jump_sign=True, shrink_corr=shrink, use_mle=use_mle, p_bounds=p_bounds, alpha_bounds=a_bounds, seed=seed,
                   nthreads=2)
    assert np.all(got["moves"] > 0) and got["sample_beta"].shape == (m2, 2, 2)
    for g, (p_init, st) in enumerate(zip(p_inits, streams)):
        UZ = [grid_ref.draws(seed, st, k, m2) for k in range(burn + it)]
        p_draws = [[ref.next_p(nb, m2, mean_ld, p_bounds, seed, st, k) for nb in range(m2 + 1)] for k in range(burn + it)]
        boot = [[ref.boot(nb, seed, st, k) for nb in range(m2 + 1)] for k in range(burn + it)]
        want = ref.py_auto_one(p, i, x, m2, bh, nv, lv, None, p_init, 0.3, burn, it, step, True, shrink, use_mle, p_bounds,
                               (a_bounds[0] + 1, a_bounds[1] + 1), [u for u, _ in UZ], [z for _, z in UZ], p_draws, boot)
        for key, name in (("beta_est", "beta_est"), ("postp_est", "postp_est"), ("corr_est", "corr_est"),
                          ("path_p_est", "path_p"), ("path_h2_est", "path_h2"), ("path_alpha_est", "path_alpha")):
            assert np.array_equal(want[key], got[name][:, g], equal_nan=True), (key, g)
        assert np.array_equal(want["sample_beta"], got["sample_beta"][:, :, g])
        assert np.isfinite(want["beta_est"]).all() and np.any(want["sample_beta"][:, 1] != 0)
        assert np.all(np.isnan(want["path_alpha_est"])) == (not use_mle)
        assert np.all(got["path_nb"][:, g] > 0)


def test_the_sums_of_the_mle_have_the_restatements_order():
    rng = np.random.default_rng(0)
    for nb in (1, 255, 256, 257, 513):
        a, b = rng.normal(0, 1.5, nb), rng.gamma(1.0, 1e-4, nb)
        assert list(ref.sums(a, b, 0.37)) == ref.py_sums(a, b, 0.37)


# ---- the MLE ------------------------------------------------------------------------------------------------------------------

def _objective(a, b, alpha1, sigma2):
    """src/optim-MLE-alpha.h:38-48 with exactly rounded sums"""
    return alpha1 * math.fsum(a) + a.size * math.log(sigma2) + math.fsum(b * np.exp(-alpha1 * a)) / sigma2


def test_mle_is_the_minimiser_over_the_box():
    """About 200 random problems.  The objective at the result has to be <= f(q) + 1e-9 |f(q)| for the end point q of
    scipy's L-BFGS-B from the same start and for every q of a 201 x 201 grid of the box: an exact minimiser cannot lose
    to a feasible point, and 1e-9 |f| is the rounding margin of the nb-term sums, not a measured quantity.  The margin
    is taken on |f(q)|: with sigma2 around 1e-4 the objective is negative, and f(q) (1 + 1e-9) would then ask the result
    to beat every feasible point by a margin, which no minimiser can."""
    rng = np.random.default_rng(11)
    sizes = [1, 255, 256, 257, 513] + [int(v) for v in rng.integers(2, 400, 195)]
    for case, nb in enumerate(sizes):
        a = rng.normal(rng.normal(0, 1), rng.uniform(0.2, 1.5), nb)           # log variances: varying
        b = rng.gamma(rng.uniform(0.5, 2), 1.0, nb) * 10.0 ** rng.uniform(-6, 0)  # squared effects
        lo = rng.uniform(-0.5, 0.9)
        bounds = (lo, lo + rng.uniform(0.05, 2.0))
        # the previous sigma2: near the scale of b at times, far from it at others, so that all of the box's faces occur
        sig_prev = float(np.mean(b * np.exp(-rng.uniform(*bounds) * a))) * 10.0 ** rng.choice([0, 0, -1, 1, 0.2, -0.2])
        start = np.array([rng.uniform(*bounds), sig_prev])
        got = ref.mle(a, b, bounds, start)
        assert bounds[0] <= got[0] <= bounds[1] and sig_prev / 2 <= got[1] <= sig_prev * 2, case
        f_got = _objective(a, b, got[0], got[1])
        box = [bounds, (sig_prev / 2, sig_prev * 2)]
        res = optimize.minimize(lambda q: _objective(a, b, q[0], q[1]), start, method="L-BFGS-B", bounds=box,
                                jac=lambda q: np.array([np.sum(a) - np.sum(a * b * np.exp(-q[0] * a)) / q[1],
                                                        (nb - np.sum(b * np.exp(-q[0] * a)) / q[1]) / q[1]]))
        q = np.clip(res.x, [box[0][0], box[1][0]], [box[0][1], box[1][1]])
        f_q = _objective(a, b, q[0], q[1])
        assert f_got <= f_q + 1e-9 * abs(f_q), (case, nb, got, q, f_got, f_q)
        al = np.linspace(bounds[0], bounds[1], 201)
        sg = np.linspace(box[1][0], box[1][1], 201)
        S = np.array([math.fsum(b * np.exp(-v * a)) for v in al])
        F = al[:, None] * math.fsum(a) + nb * np.log(sg)[None, :] + S[:, None] / sg[None, :]
        assert np.all(f_got <= F + 1e-9 * np.abs(F)), (case, nb, got, f_got, F.min())


def test_mle_edge_cases():
    rng = np.random.default_rng(3)
    assert list(ref.mle([], [], (-0.5, 1.5), [0.25, 3e-4])) == [0.25, 3e-4]          # nb = 0: par as it was
    a, b = rng.normal(0, 1, 40), rng.gamma(1.0, 1e-4, 40)
    got = ref.mle(a, b, (0.0, 0.0), [0.7, 1e-4])                                     # alpha_lo == alpha_hi
    assert got[0] == 0.0 and got[1] == min(max(ref.sums(a, b, 0.0)[1] / 40, 0.5e-4), 2e-4)
    # the restatement in Python gives the same bits, bounds and interior
    for bounds, sig in (((-0.5, 1.5), 1e-4), ((0.9, 1.0), 1e-4), ((-0.5, -0.4), 1e-2), ((-0.5, 1.5), 1e-7)):
        assert list(ref.mle(a, b, bounds, [0.0, sig])) == ref.py_mle(a, b, bounds[0], bounds[1], [0.0, sig])


# ---- rbeta ----------------------------------------------------------------------------------------------------------------------

def test_log_det_on_the_arguments_of_the_gamma_draw():
    """gibbs_step.hpp documents log_det on (2^-53, 0.075]; Marsaglia and Tsang's acceptance calls it on a uniform, up to
    1 - 2^-53, and on (1 + c Z)^3, between 2^-159 and 5^3: within 1e-13 relative of libm there too (absolute 1e-16 next
    to 1, where the logarithm itself vanishes)."""
    x = np.concatenate([np.exp(np.linspace(math.log(2.0 ** -159), math.log(125.0), 200001)), np.linspace(0.5, 2.0, 100001),
                        1 - 2.0 ** -53 * np.arange(1, 2000, 2), 1 + 2.0 ** -52 * np.arange(1, 2000)])
    got, want = grid_ref.log_det(x), np.log(x)
    assert np.all(np.abs(got - want) <= 1e-13 * np.abs(want) + 1e-16)


@pytest.mark.parametrize("a,b", [(1.0, 1.0), (1.0, 4000.0), (37.5, 812.25)])
def test_rbeta_moments(a, b):
    """20 000 draws: the mean within 5 standard errors of a / (a + b), the variance within 5 of its own.  With
    mu_k the central moments of Beta(a, b): se(mean) = sqrt(mu_2 / n), se(var) = sqrt((mu_4 - mu_2^2) / n)."""
    n = 20000
    x = ref.rbeta(a, b, n, seed=2024, stream=3)
    assert x.min() > 0 and x.max() < 1
    mean = a / (a + b)
    var = a * b / ((a + b) ** 2 * (a + b + 1))
    kurt = 3 + 6 * ((a - b) ** 2 * (a + b + 1) - a * b * (a + b + 2)) / (a * b * (a + b + 2) * (a + b + 3))
    assert abs(x.mean() - mean) < 5 * math.sqrt(var / n)
    assert abs(x.var() - var) < 5 * math.sqrt((kurt - 1) * var ** 2 / n)
    # the same counter gives the same bits, another one does not
    assert np.array_equal(ref.rbeta(a, b, 100, seed=2024, stream=3, sweep0=50), x[50:150])
    assert not np.any(ref.rbeta(a, b, 100, seed=2025, stream=3) == x[:100])
    assert not np.any(ref.rbeta(a, b, 100, seed=2024, stream=4) == x[:100])


def test_next_p_is_rbeta_clamped():
    x = ref.rbeta(1 + 12 / 3.5, 1 + (400 - 12) / 3.5, 1, seed=9, stream=2, sweep0=17)[0]
    assert ref.next_p(12, 400, 3.5, (1e-5, 1.0), 9, 2, 17) == x
    assert ref.next_p(12, 400, 3.5, (0.5, 0.6), 9, 2, 17) == 0.5 and ref.next_p(12, 400, 3.5, (1e-5, 1e-4), 9, 2, 17) == 1e-4


# ---- bootstrap and counters ---------------------------------------------------------------------------------------------------

def test_bootstrap_index_stays_below_nb():
    top = 1 - 2.0 ** -53                                   # the largest uniform
    for nb in (1, 2, 2 ** 31 - 1):
        assert ref.boot_pick(nb, top) == nb - 1
        assert ref.boot_pick(nb, 2.0 ** -53) == 0
    assert ref.boot_pick(2 ** 31 - 1, 0.5) == 2 ** 30 - 1
    idx = ref.boot(1000, 5, 6, 7)
    assert idx.min() >= 0 and idx.max() < 1000 and np.unique(idx).size > 500
    assert np.array_equal(idx[:10], ref.boot(1000, 5, 6, 7)[:10])


def test_tagged_counters_collide_with_no_coordinate_counter():
    """a counter is (word 0, sweep word, stream): coordinates use sweep words below 2^30, the epilogue's three purposes
    set the two top bits.  The four sets of sweep words are disjoint, on a small range and at the ends of the full one."""
    sweeps = list(range(0, 300)) + [2 ** 30 - 1 - k for k in range(300)]
    words = {tag: {ref.tagged_sweep(s, tag) for s in sweeps} for tag in range(4)}
    assert words[0] == set(sweeps)
    for t in range(4):
        assert len(words[t]) == len(sweeps)
        assert all(w >> 30 == t for w in words[t])
        for u in range(t + 1, 4):
            assert not (words[t] & words[u])
    # the draws themselves: the first gamma's attempts, the second's and the bootstrap's differ from the coordinates'
    U0, _ = grid_ref.draws(1, 2, 5, 64)
    for tag in (1, 2, 3):
        U, _ = grid_ref.draws(1, 2, ref.tagged_sweep(5, tag), 64)
        assert not np.any(U == U0)


# ---- the argument checks of snp_ldpred2_auto -------------------------------------------------------------------------------

def test_argument_errors_come_before_any_device_work():
    import bigsnpr_amd as ba
    from scipy import sparse
    m2 = 30
    A = sparse.csc_matrix(banded_corr(m2, 3, seed=2))
    rng = np.random.default_rng(1)
    df = {"beta": rng.normal(0, 0.05, m2), "beta_se": np.full(m2, 0.03), "n_eff": np.full(m2, 1500.0)}
    with pytest.raises(ValueError, match="'df_beta' should have element 'beta'."):
        ba.snp_ldpred2_auto(A, {k: v for k, v in df.items() if k != "beta"}, 0.3)
    with pytest.raises(ValueError, match="'h2_init' should have only positive values."):
        ba.snp_ldpred2_auto(A, df, 0.0)
    with pytest.raises(ValueError, match="Arguments should have the same length"):
        ba.snp_ldpred2_auto(A, {k: v[:-1] for k, v in df.items()}, 0.3)
    with pytest.raises(ValueError, match="ind.corr %in% cols_along"):
        ba.snp_ldpred2_auto(A, df, 0.3, ind_corr=np.arange(1, m2 + 1))
    with pytest.raises(ValueError, match="'df_beta\\$beta_se' should have only positive values."):
        ba.snp_ldpred2_auto(A, dict(df, beta_se=np.zeros(m2)), 0.3)
    with pytest.raises(ValueError, match="'report_step' should be at least 1."):
        ba.snp_ldpred2_auto(A, df, 0.3, report_step=0)
    with pytest.raises(ValueError, match="below 2\\^30"):
        ba.snp_ldpred2_auto(A, df, 0.3, burn_in=2 ** 29, num_iter=2 ** 29)
    with pytest.raises(ValueError, match="'stream' should be in"):
        ba.snp_ldpred2_auto(A, df, 0.3, stream=[2 ** 63])
