"""AUC / AUCBoot / pcor / big_prodMat / snp_grid_AUC without a GPU: the CPU statement (tests/native/auc_ref.cpp over
auc_step.hpp, the header the kernels of auc.hip are compiled from) against the O(n1 n0) definition in numpy integers, its
draws against a numpy restatement of the resample rule with the Philox of tests/test_impute_cpu.py, its replicates against
the definition on the resampled vectors, the header under a sanitizer as a stand-alone program, and the argument checks of
the host mirror, none of which needs a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import auc_ref as ref  # noqa: E402
from test_impute_cpu import philox4x32_10  # noqa: E402


def cases():
    """(name, scores, target): the case list of the issue"""
    rng = np.random.default_rng(11)
    out = []
    for n in (2, 17, 257, 600):
        y = rng.integers(0, 2, n)
        y[0], y[1] = 0, 1
        out.append(("random doubles %d" % n, rng.normal(size=n), y))
        for L in (2, 3, 17):
            out.append(("lattice %d of %d" % (L, n), rng.integers(0, L, n).astype(np.float64) - 1.0, y))
        out.append(("all equal %d" % n, np.full(n, 0.25), y))
        out.append(("-0.0 beside +0.0 %d" % n, np.where(rng.integers(0, 2, n) == 1, -0.0, 0.0), y))
        out.append(("+-Inf %d" % n, rng.choice([-np.inf, np.inf, -0.0, 0.0, 1.5, -1.5], n), y))
    out.append(("one case, one control", np.array([1.0, 0.0]), np.array([1, 0])))
    out.append(("one case, one control, reversed", np.array([0.0, 1.0]), np.array([1, 0])))
    out.append(("one case, one control, zeros", np.array([-0.0, 0.0]), np.array([1, 0])))
    return out


@pytest.mark.parametrize("name,x,y", cases(), ids=[c[0] for c in cases()])
def test_twin_against_the_definition(name, x, y):
    r = ref.auc(x, y)
    two_u, n1, n0 = ref.two_u_definition(x, y)
    assert np.array_equal(r["counts"][0], np.array([two_u, n1, n0], dtype=np.uint64))
    assert np.array_equal(r["auc"], np.array([ref.auc_definition(x, y)]))


def test_twin_values_that_can_be_stated_by_hand():
    assert ref.auc([0.0, 1.0], [0, 1])["auc"][0] == 1.0
    assert ref.auc([1.0, 0.0], [0, 1])["auc"][0] == 0.0
    assert ref.auc([-0.0, 0.0], [0, 1])["auc"][0] == 0.5
    assert ref.auc(np.full(9, 3.0), [0, 1, 0, 1, 1, 0, 0, 0, 1])["auc"][0] == 0.5
    assert ref.auc([-np.inf, np.inf, 0.0, np.inf], [0, 1, 0, 1])["auc"][0] == 1.0
    # several columns share the target; a NaN column is named
    X = np.array([[0.0, 2.0], [1.0, 1.0], [2.0, 0.0]])
    assert np.array_equal(ref.auc(X, [0, 0, 1])["auc"], [1.0, 0.0])
    X[1, 1] = np.nan
    with pytest.raises(ValueError, match="column 1"):
        ref.auc(X, [0, 0, 1])


def test_keys_order_the_doubles():
    lib = ref.load()
    v = np.array([-np.inf, -1e300, -1.5, -5e-324, -0.0, 0.0, 5e-324, 1.5, 1e300, np.inf])
    k = [lib.auc_order_key(float(a)) for a in v]
    assert k[4] == k[5]
    assert all(a < b for a, b in zip(k[:4], k[1:5])) and all(a < b for a, b in zip(k[5:-1], k[6:]))
    assert lib.auc_draw_tag() == ref.TAG


@pytest.mark.parametrize("n,b,seed", [(1, 0, 0), (6, 3, 7), (1000, 63, 2 ** 63 + 12345), (70001, 5, 0xFFFFFFFFFFFFFFFF)])
def test_draws_of_the_twin(n, b, seed):
    got = ref.draws(n, b, seed)
    assert np.array_equal(got, ref.philox_rows(philox4x32_10, n, b, seed))
    assert got.min() >= 0 and got.max() < n


def test_draws_are_uniform_and_differ_between_replicates():
    n = 1000
    rows = np.concatenate([ref.draws(n, b, 5) for b in range(200)])
    cnt = np.bincount(rows, minlength=n)
    chi2 = ((cnt - 200.0) ** 2 / 200.0).sum()          # 999 degrees of freedom: mean 999, sd 44.7
    assert 999 - 5 * 44.7 < chi2 < 999 + 5 * 44.7
    assert not np.array_equal(ref.draws(n, 0, 5), ref.draws(n, 1, 5))
    assert not np.array_equal(ref.draws(n, 0, 5), ref.draws(n, 0, 6))


@pytest.mark.parametrize("n,nboot,one_case", [(6, 64, True), (300, 40, False)])
def test_replicates_of_the_twin(n, nboot, one_case):
    rng = np.random.default_rng(n)
    x = np.column_stack([rng.normal(size=n), rng.integers(0, 3, n).astype(np.float64)])
    y = np.zeros(n, dtype=np.int64)
    if one_case:
        y[2] = 1
    else:
        y[rng.choice(n, n // 3, replace=False)] = 1
    rep = ref.boot(x, y, nboot, 99)
    for b in range(nboot):
        rows = ref.philox_rows(philox4x32_10, n, b, 99)
        for j in range(2):
            want = ref.auc_definition(x[rows, j], y[rows])
            assert rep[b, j] == want or (np.isnan(rep[b, j]) and np.isnan(want)), (b, j)
    if one_case:
        # P(no case among 6 draws) = (5/6)^6 = 0.335
        assert 0.15 < np.isnan(rep[:, 0]).mean() < 0.55
        assert np.array_equal(np.isnan(rep[:, 0]), np.isnan(rep[:, 1]))


def test_header_under_a_sanitizer(tmp_path):
    exe = str(tmp_path / "auc_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-ffp-contract=off", "-std=c++17",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "bigsnpr_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "native"),
                           os.path.join(ROOT, "tests", "native", "auc_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks held" in out.stdout


# ---- the host mirror: statistics and argument checks, no device ---------------------------------------------------------------
@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def test_boot_statistics(ba):
    rng = np.random.default_rng(3)
    rep = rng.uniform(size=(500, 3))
    rep[::7, 1] = np.nan
    rep[:, 2] = np.nan
    st = ba.boot_statistics(rep)
    v = rep[:, 1][~np.isnan(rep[:, 1])]
    assert np.array_equal(st[0], [rep[:, 0].mean(), *np.quantile(rep[:, 0], [0.025, 0.975]), rep[:, 0].std(ddof=1)])
    assert np.array_equal(st[1], [v.mean(), *np.quantile(v, [0.025, 0.975]), v.std(ddof=1)])
    assert np.isnan(st[2]).all()
    # R's type 7 on a case that can be done by hand: quantile(0:4, 0.025) = 0.1
    assert np.isclose(ba.boot_statistics(np.arange(5.0)[:, None])[0, 1], 0.1, rtol=0, atol=1e-15)


def test_auc_argument_checks(ba):
    x = np.arange(6.0)
    with pytest.raises(ValueError, match="'pred' and 'target' should have the same length"):
        ba.AUC(x, [0, 1, 0])
    with pytest.raises(ValueError, match="'target' should hold 0 and 1 only"):
        ba.AUC(x, [2, 2, 2, 2, 2, 2])
    with pytest.raises(ValueError, match="'target' should hold 0 and 1 only"):
        ba.AUC(x, [0, 1, 0, 1, 0, np.nan])
    with pytest.raises(ValueError, match="'target' should hold both classes"):
        ba.AUC(x, np.zeros(6))
    with pytest.raises(ValueError, match="'target' should hold both classes"):
        ba.AUC(x, np.ones(6))
    X = np.zeros((6, 4))
    X[3, 2] = X[0, 3] = np.nan
    with pytest.raises(ValueError, match=r"missing value \(NaN\) in 'pred', first in column 2"):
        ba.AUC(X, [0, 1, 0, 1, 0, 1])
    with pytest.raises(ValueError, match="first in column 3"):          # the NaN of column 2 is not among the rows
        ba.AUC(X, [0, 1, 0], ind_row=[0, 1, 2])
    with pytest.raises(ValueError, match="'ind_row' out of bounds"):
        ba.AUC(x, [0, 1], ind_row=[0, 6])
    with pytest.raises(ValueError, match="should be a vector or a matrix"):
        ba.AUC(np.zeros((2, 2, 2)), [0, 1])
    with pytest.raises(ValueError, match="at least one row and one column"):
        ba.AUC(np.zeros((0, 2)), [])


def test_aucboot_argument_checks(ba):
    x = np.arange(6.0)
    y = [0, 1, 0, 1, 0, 1]
    with pytest.raises(ValueError, match="'nboot' should be between 1 and"):
        ba.AUCBoot(x, y, nboot=0)
    with pytest.raises(ValueError, match="'seed' should be between 0 and"):
        ba.AUCBoot(x, y, seed=-1)
    with pytest.raises(ValueError, match="'seed' should be between 0 and"):
        ba.AUCBoot(x, y, seed=2 ** 64)
    with pytest.raises(ValueError, match="'target' should hold both classes"):
        ba.AUCBoot(x, np.zeros(6))
    with pytest.raises(ValueError, match="first in column 0"):
        ba.AUCBoot(np.r_[x[:5], np.nan], y)


def test_grid_auc_argument_checks(ba):
    y = [0, 1, 0, 1]
    with pytest.raises(ValueError, match="'n_chr' is needed for a plain matrix"):
        ba.snp_grid_AUC(np.zeros((4, 6)), y)
    with pytest.raises(ValueError, match="should be a multiple of the number of chromosomes"):
        ba.snp_grid_AUC(np.zeros((4, 7)), y, n_chr=3)
    with pytest.raises(ValueError, match="'target' should hold 0 and 1 only"):
        ba.snp_grid_AUC(np.zeros((4, 6)), [0, 1, 2, 1], n_chr=3)


def test_pcor_argument_checks(ba):
    rng = np.random.default_rng(0)
    n = 40
    x, y = rng.normal(size=(n, 2)), rng.normal(size=n)
    with pytest.raises(ValueError, match="'x' and 'y' should have the same length"):
        ba.pcor(x, y[:-1])
    with pytest.raises(ValueError, match="'x' and 'z' should have the same number of rows"):
        ba.pcor(x, y, rng.normal(size=(n - 1, 2)))
    with pytest.raises(ValueError, match=r"\[1, z\] should have at most 31 columns \(got 32\)"):
        ba.pcor(x, y, rng.normal(size=(n, 31)))
    z = rng.normal(size=(n, 3))
    z[:, 2] = z[:, 0] - 2 * z[:, 1]
    with pytest.raises(ValueError, match=r"\[1, z\] is rank-deficient"):
        ba.pcor(x, y, z)
    with pytest.raises(ValueError, match=r"\[1, z\] is rank-deficient"):
        ba.pcor(x, y, np.full((n, 1), 3.0))                  # a constant covariate beside the intercept
    for bad in (np.nan, np.inf):
        xx = x.copy()
        xx[3, 1] = bad
        with pytest.raises(ValueError, match="non-finite value"):
            ba.pcor(xx, y)
        yy = y.copy()
        yy[0] = bad
        with pytest.raises(ValueError, match="non-finite value"):
            ba.pcor(x, yy)
    with pytest.raises(ValueError, match="too few rows: n - c - 3 = 0 should be positive"):
        ba.pcor(x[:6], y[:6], rng.normal(size=(6, 3)))
    with pytest.raises(ValueError, match="'alpha' should be between 0 and 1"):
        ba.pcor(x, y, alpha=1.0)


def test_prodmat_argument_checks(ba):
    with pytest.raises(TypeError):
        ba.big_prodMat(object(), np.zeros((3, 1)))
