"""What the tests of snp_ldpred2_auto share: the CPU statement (tests/native/ldpred2_auto_ref.cpp) finished as
R/LDpred2.R:257-264 finishes a chain, and the comparison of every returned array and scalar, bit for bit.  There is no
tolerance anywhere in this file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import ldpred2_auto_ref as ref  # noqa: E402

ARRAYS = ("beta_est", "postp_est", "corr_est", "sample_beta", "path_p_est", "path_h2_est", "path_alpha_est")
SCALARS = ("h2_est", "p_est", "alpha_est")


def expected(full, df, mean_ld, vec_p_init, h2_init, seed, sub=None, stream=None, burn_in=20, num_iter=30, report_step=None,
             allow_jump_sign=True, shrink_corr=1.0, use_MLE=True, p_bounds=(1e-5, 1.0), alpha_bounds=(-1.5, 0.5)):
    """the statement on the full columns (full = (p, i, x, m2)); df holds the rows of `sub`, mean_ld is an input (the mean
    LD score of the listed columns).  Returns the list of dicts and the statement's raw output (path_nb, moves)."""
    fp, fi, fx, m2 = full
    beta, se, n = (np.asarray(df[k]) for k in ("beta", "beta_se", "n_eff"))
    sd = 1 / np.sqrt(n * se ** 2 + beta ** 2)
    raw = ref.auto(fp, fi, fx, m2, beta * sd, n, 2 * np.log(sd), vec_p_init, h2_init, mean_ld, ind_sub=sub, stream=stream,
                   burn_in=burn_in, num_iter=num_iter, report_step=report_step, no_jump_sign=not allow_jump_sign,
                   shrink_corr=shrink_corr, use_mle=use_MLE, p_bounds=p_bounds, alpha_bounds=alpha_bounds, seed=seed, nthreads=16)
    out = []
    for g in range(len(vec_p_init)):
        out.append({"beta_est": raw["beta_est"][:, g] / sd, "postp_est": raw["postp_est"][:, g], "corr_est": raw["corr_est"][:, g],
                    "sample_beta": raw["sample_beta"][:, :, g], "path_p_est": raw["path_p"][:, g],
                    "path_h2_est": raw["path_h2"][:, g], "path_alpha_est": raw["path_alpha"][:, g],
                    "h2_est": np.mean(raw["path_h2"][burn_in:, g]), "p_est": np.mean(raw["path_p"][burn_in:, g]),
                    "alpha_est": np.mean(raw["path_alpha"][burn_in:, g])})
    return out, raw


def same(res, want):
    assert len(res) == len(want)
    for r, w in zip(res, want):
        for k in ARRAYS:
            assert np.shape(r[k]) == np.shape(w[k]), k
            assert np.array_equal(r[k], w[k], equal_nan=True), k
        for k in SCALARS:
            assert np.array_equal(r[k], w[k], equal_nan=True), k


def equal_lists(a, b):
    return len(a) == len(b) and all(np.array_equal(x[k], y[k], equal_nan=True) for x, y in zip(a, b) for k in ARRAYS + SCALARS)


def host_mean_ld(A, sub=None):
    """the mean LD score of the listed columns (src/ld-scores-sfbm.cpp: x^2 over the stored entries whose row is listed
    too), summed on the host: for the proofs that run without a device.  The GPU tests pass the device's own mean"""
    As = A if sub is None else A[sub][:, sub]
    return float(np.mean(np.asarray(As.multiply(As).sum(axis=0)).ravel()))
