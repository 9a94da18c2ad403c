"""The header statement of the OADP projection (bigsnpr_amd/csrc/oadp_step.hpp through tests/native/oadp_ref.cpp: the code
the kernel compiles from, run by one lane) against pca_OADP_proj2 of bigsnpr_amd/prs.py and against the brute-force
definition (append the sample to a rank-K reference, redo the PCA, Procrustes over ALL reference samples).

The tolerance is the one of the project's two existing OADP comparisons: rtol = 1e-9, atol = 1e-9 d[0].

K in {1, 2, 20, the cap}; a zero sample, |y|^2 = |l|^2 exactly, |y|^2 just below |l|^2, |y|^2 > 9 d_1^2, two equal
singular values; a NaN row comes back NaN (and the call comes back); a zero, a negative, a NaN or an infinite singular
value and K above the cap are errors.  No GPU, no library."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oadp_inputs as inp  # noqa: E402
import oadp_ref as ref  # noqa: E402

CAP = ref.max_k()
KS = (1, 2, 20, CAP)
N = 24


def _host():
    # prs.py imports the package (which needs the built library only when called): load the one function from source
    src = open(os.path.join(ROOT, "bigsnpr_amd", "prs.py")).read()
    start = src.index("def pca_OADP_proj2(")
    end = src.index("\ndef ", start + 10)
    ns = {"np": np}
    exec(src[start:end], ns)
    return ns["pca_OADP_proj2"]


def _brute(Xk, U, d, y, K):
    aug = np.vstack([Xk, y[None, :]])
    Ua, sa, _ = np.linalg.svd(aug, full_matrices=False)
    scores = Ua[:, :K] * sa[:K]
    ref_aug, new_aug = scores[:-1], scores[-1]
    target = U * d
    Up, sp, Vtp = np.linalg.svd(ref_aug.T @ target)
    R = Up @ Vtp
    rho = sp.sum() / (ref_aug ** 2).sum()
    return rho * new_aug @ R


def _close(got, want, d):
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * d[0])


def test_cap_is_at_least_50():
    assert CAP >= 50


@pytest.mark.parametrize("equal_pair", (False, True))
@pytest.mark.parametrize("K", KS)
def test_statement_equals_pca_oadp_proj2(K, equal_pair):
    d = inp.sval(K, seed=K, equal_pair=equal_pair)
    XV, X_norm, rows = inp.batch(N, d, seed=10 + K)
    assert set(rows.values()) == set(inp.EDGE_KINDS)
    got, sweeps = ref.proj(XV, X_norm, d, return_sweeps=True)
    ok = inp.finite_rows(N, rows)
    _close(got[ok], _host()(XV[ok], X_norm[ok], d), d)
    # a NaN row: NaN, and nothing else is
    assert np.isnan(got[~ok]).all() and (~ok).sum() == 2
    assert np.isfinite(got[ok]).all()
    # no sample ran into the sweep cap: the absolute floor ends the sweeps of a sample in the span of the PCs
    assert sweeps[ok].max() < ref.sweep_cap() and sweeps[ok].min() >= 0
    zero = [i for i, kind in rows.items() if kind == "zero"]
    assert np.array_equal(got[zero], np.zeros((len(zero), K)))


@pytest.mark.parametrize("K", KS)
def test_statement_equals_the_definition_on_a_rank_k_reference(K):
    rng = np.random.default_rng(77 + K)
    n_ref, p = 80, 100
    U = np.linalg.qr(rng.normal(size=(n_ref, K)))[0]
    Q = np.linalg.qr(rng.normal(size=(p, K + 1)))[0]
    V, q = Q[:, :K], Q[:, K]
    d = inp.sval(K, seed=5 + K, equal_pair=True)
    Xk = (U * d) @ V.T
    XV, X_norm, rows = inp.batch(12, d, seed=3 + K)
    got = ref.proj(XV, X_norm, d)
    for i in np.nonzero(inp.finite_rows(12, rows))[0]:
        y = V @ XV[i] + np.sqrt(max(X_norm[i] - XV[i] @ XV[i], 0.0)) * q
        _close(got[i], _brute(Xk, U, d, y, K), d)


def test_unsorted_singular_values_are_sorted_by_the_statement():
    d = inp.sval(6, seed=1)[::-1].copy()      # ascending: the selection must not rely on the order of d
    XV, X_norm, rows = inp.batch(N, d, seed=4)
    ok = inp.finite_rows(N, rows)
    got = ref.proj(XV, X_norm, d)
    np.testing.assert_allclose(got[ok], _host()(XV[ok], X_norm[ok], d), rtol=1e-9, atol=1e-9 * d.max())


def test_nan_and_infinite_norms_return_nan_rows():
    d = inp.sval(5, seed=2)
    XV, X_norm, _ = inp.batch(4, d, seed=8)
    XV[:] = np.abs(XV) + 1.0
    X_norm[:] = (XV ** 2).sum(axis=1) * 2.0
    X_norm[1] = np.nan
    X_norm[2] = np.inf
    XV[3, 0] = -np.inf
    got = ref.proj(XV, X_norm, d)
    assert np.isfinite(got[0]).all() and np.isnan(got[1:]).all()


@pytest.mark.parametrize("bad", (0.0, -3.0, np.nan, np.inf))
def test_singular_values_must_be_finite_and_positive(bad):
    d = inp.sval(4, seed=3)
    d[2] = bad
    XV, X_norm, _ = inp.batch(3, inp.sval(4, seed=3), seed=1)
    with pytest.raises(ValueError, match="singular values must be finite and positive"):
        ref.proj(XV, X_norm, d)


def test_k_above_the_cap_is_an_error():
    K = CAP + 1
    d = inp.sval(K, seed=0)
    XV, X_norm, _ = inp.batch(2, d, seed=0)
    with pytest.raises(ValueError, match="more than %d singular values" % CAP):
        ref.proj(XV, X_norm, d)
