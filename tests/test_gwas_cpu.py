"""big_univLinReg / big_univLogReg without a GPU: the CPU statement (tests/native/gwas_ref.cpp over irls_step.hpp, the header
the kernel is compiled from) against the oracle's logistic scan and against numpy's least squares, the pieces of
irls_step.hpp under a sanitizer as a stand-alone program, and the argument errors of the host mirror."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

import gwas_ref as ref  # noqa: E402


def _y01(golden_dir):
    return np.array([int(line.split()[5]) for line in open(os.path.join(golden_dir, "example.fam"))]) - 1.0


@pytest.fixture(scope="module")
def data(orc, golden_dir, example_bed):
    """decoded example data (517 x 4542, complete), the case / control phenotype and the leading 10 left singular vectors"""
    X = orc.read_bed(example_bed, na_val=3).astype(np.float64)
    assert not (X == 3).any()
    u = orc.dense_svd(example_bed, None, None, k=10)["u"]
    return dict(X=np.asfortranarray(X), y=_y01(golden_dir), u=u, G=orc.fbm_from_bed(example_bed))


def test_logistic_statement_agrees_with_the_oracle(orc, data):
    got = ref.logreg(data["X"], data["y"], data["u"])
    want = orc.univ_logreg(data["G"], data["y"], data["u"])
    # every variant of this input converges, in 3 to 5 solves: none is left out of the comparison
    assert got["niter"].min() >= 3 and got["niter"].max() <= 6
    d_est = np.abs(got["estim"] - want["estim"]) / want["std_err"]
    d_se = np.abs(got["std_err"] / want["std_err"] - 1)
    print("max |d estim| / std_err = %.3g, max rel d std_err = %.3g" % (d_est.max(), d_se.max()))
    assert d_est.max() <= 1e-9
    assert d_se.max() <= 1e-7


def test_linear_statement_agrees_with_lstsq(data):
    rng = np.random.default_rng(7)
    X, u = data["X"], data["u"]
    n = X.shape[0]
    y = rng.standard_normal(n) + 0.3 * X[:, 11]
    cols = np.arange(0, X.shape[1], 7)
    got = ref.linreg(X[:, cols], y, u)
    assert got["df"] == n - 11 - 1
    est, se = np.empty(cols.size), np.empty(cols.size)
    for t, j in enumerate(cols):
        A = np.column_stack([X[:, j], np.ones(n), u])
        b, res, rank, _ = np.linalg.lstsq(A, y, rcond=None)
        assert rank == A.shape[1]
        est[t] = b[0]
        se[t] = np.sqrt(res[0] / (n - A.shape[1]) * np.linalg.inv(A.T @ A)[0, 0])
    np.testing.assert_allclose(got["estim"], est, rtol=1e-7, atol=0)
    np.testing.assert_allclose(got["std_err"], se, rtol=1e-7, atol=0)


def test_thr_eigval_drops_a_duplicated_covariate(data):
    X, u = data["X"][:, :200], data["u"][:, :4]
    rng = np.random.default_rng(8)
    y = rng.standard_normal(X.shape[0])
    dup = np.column_stack([u, u[:, 1]])
    assert ref.covar_basis(u, X.shape[0]).shape[1] == 5 and ref.covar_basis(dup, X.shape[0]).shape[1] == 5
    a, b = ref.linreg(X, y, u), ref.linreg(X, y, dup)
    assert a["df"] == b["df"]
    np.testing.assert_allclose(b["estim"], a["estim"], rtol=1e-10)
    np.testing.assert_allclose(b["std_err"], a["std_err"], rtol=1e-10)
    from bigsnpr_amd.gwas import covar_basis
    assert covar_basis(dup).shape[1] == 5
    np.testing.assert_allclose(covar_basis(dup) @ covar_basis(dup).T, covar_basis(u) @ covar_basis(u).T, atol=1e-12)


def test_edges_of_the_statement():
    """a monomorphic variant and one with a missing value: NaN, niter = 0; a variant carried only by cases: niter = -1
    with finite outputs (quasi-complete separation: the coefficient grows by about one per solve)"""
    rng = np.random.default_rng(9)
    n = 300
    y = (rng.random(n) < 0.4).astype(np.float64)
    X = rng.integers(0, 3, size=(n, 5)).astype(np.float64)
    X[:, 1] = 2.0
    X[5, 2] = np.nan
    X[:, 3] = 0.0
    X[np.flatnonzero(y == 1)[:20], 3] = 1.0
    cov = rng.standard_normal((n, 3))
    r = ref.logreg(X, y, cov)
    assert list(r["niter"][[1, 2, 3]]) == [0, 0, -1] and r["niter"][0] > 0 and r["niter"][4] > 0
    assert np.isnan(r["estim"][[1, 2]]).all() and np.isnan(r["std_err"][[1, 2]]).all()
    assert np.isfinite(r["estim"][[0, 3, 4]]).all() and np.isfinite(r["std_err"][[0, 3, 4]]).all()
    lin = ref.linreg(X, rng.standard_normal(n), cov)
    assert np.isnan(lin["estim"][[1, 2]]).all() and np.isfinite(lin["estim"][[0, 3, 4]]).all()


def test_sample_map_against_libm_and_in_the_tails():
    eta = np.concatenate([np.linspace(-40, 40, 4001), [-745.0, -700.0, 700.0, 745.0]])
    for y in (0.0, 1.0):
        w, wz = ref.sample_map(eta, np.full(eta.size, y))
        # the reference from exp(-|eta|), so that neither p nor 1 - p loses its digits in a tail
        e = np.exp(-np.abs(eta))
        big, small = 1.0 / (1.0 + e), e / (1.0 + e)
        p, omp = np.where(eta < 0, small, big), np.where(eta < 0, big, small)
        np.testing.assert_allclose(w, big * small, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(wz, big * small * eta + (omp if y == 1.0 else -p), rtol=1e-12, atol=1e-300)
        assert np.isfinite(wz).all() and (w >= 0).all()


def test_irls_step_under_a_sanitizer(tmp_path):
    """solve, inverse and convergence rule on hand-made systems (P = 2, 16, 17, 32; one singular) as a stand-alone program
    built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "irls_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-ffp-contract=off", "-std=c++17",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "bigsnpr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "irls_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks held" in out.stdout


def test_argument_errors_need_no_gpu():
    import bigsnpr_amd as ba
    G = types.SimpleNamespace(nrow=20, ncol=5)   # the checks come before the image is looked at
    y = np.arange(20) % 2.0
    with pytest.raises(ba.BsnError, match="composed of 0s and 1s"):
        ba.big_univLogReg(G, np.where(y == 1, 2.0, 0.0))
    with pytest.raises(ba.BsnError, match="Incompatibility between dimensions"):
        ba.big_univLogReg(G, y, covar_train=np.zeros((19, 2)))
    with pytest.raises(ba.BsnError, match="Incompatibility between dimensions"):
        ba.big_univLinReg(G, y, covar_train=np.zeros((21, 2)))
    with pytest.raises(ba.BsnError, match="'maxiter' must be at least 1"):
        ba.big_univLogReg(G, y, maxiter=0)
    with pytest.raises(ba.BsnError, match="more than 30 columns"):
        ba.big_univLogReg(G, y, covar_train=np.zeros((20, 31)))
    with pytest.raises(ba.BsnError, match="more than 30 columns"):
        ba.big_univLinReg(G, y, covar_train=np.zeros((20, 31)))
    with pytest.raises(ba.BsnError, match="same length"):
        ba.big_univLogReg(G, y[:10], ind_train=np.arange(12))
