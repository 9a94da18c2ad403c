"""The cases of tests/test_gpu_plr_shapes.py on the CPU statement alone (tests/native/plr_ref.cpp), forward and reversed row
sums: the discrete outputs of the two orders agree, and the condition each case is named for (the loop turn or branch of
bigsnpr_amd/csrc/plr.hip it is meant to reach) holds in both.  A device test on these inputs therefore
cannot pass without reaching its branch."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import plr_ref as ref  # noqa: E402
import plr_inputs as inp  # noqa: E402

FAMILIES = inp.FAMILIES


def two_orders(case, family, **over):
    """the statement in both orders, their discrete outputs equal; returns both"""
    kw = inp.ref_kw(case, family, **over)
    out = [ref.fit(case["X"], case["ys"][family], case["fold"], case["K"], reverse=rev, **kw) for rev in (False, True)]
    f, r = out
    for k in ("status", "n_done", "best", "iter", "nb_active", "turns"):
        assert np.array_equal(f[k], r[k]), (case["name"], family, k, f[k], r[k])
    assert np.array_equal(f["beta"] != 0, r["beta"] != 0), (case["name"], family)
    return out


def test_turns_counts_the_sweeps_after_the_start():
    """one sweep per lambda when nothing ever enters (H: a grid of zeros), at least one per lambda otherwise, none at l = 0"""
    for f in two_orders(inp.case_monomorphic(False), "linear"):
        assert np.array_equal(f["turns"], f["n_done"] - 1)
    for f in two_orders(inp.case_max_iter(1), "linear"):
        assert np.array_equal(f["turns"], f["n_done"] - 1)          # one pass, then the cap closes the lambda
    for f in two_orders(inp.case_lambda_max_past_1024(), "linear"):
        assert (f["turns"] > f["n_done"] - 1).all()                 # a lambda at which a column enters takes two turns


@pytest.mark.parametrize("family", FAMILIES)
def test_a_active_set_crosses_1024(family):
    for f in two_orders(inp.case_active_set_across_1024(), family):
        assert set(f["status"]) == {4}
        nb = f["nb_active"]
        print(family, "nb_active at l = 1, 6, 11:", nb[1], nb[6], nb[11], "iter", f["iter"].max())
        for c in range(2):
            below = np.nonzero(nb[1:, c] < 1024)[0]
            above = np.nonzero(nb[1:, c] > 1024)[0]
            assert below.size and above.size and above.max() > below.min(), nb[:, c]


@pytest.mark.parametrize("family", FAMILIES)
def test_b_lambda_max_comes_from_a_column_past_1024(family):
    case = inp.case_lambda_max_past_1024()
    for f in two_orders(case, family):
        for c in range(2):
            first = inp.lambda_max_below(case, family, c, 1024)
            whole = inp.lambda_max_below(case, family, c, 1200)
            print(family, c, "lambda_max", f["lambda"][0, c], "numpy: all columns", whole, "columns < 1024", first)
            assert abs(whole / f["lambda"][0, c] - 1) < 1e-12      # the restatement is the statement's lambda_max
            assert first < 0.9 * f["lambda"][0, c]
            assert f["beta"][1090, c] != 0


@pytest.mark.parametrize("family", FAMILIES)
def test_c_chain_blocks_die_in_both_orders(family):
    for f in two_orders(inp.case_chain_blocks(0), family):
        t = f["turns"]
        print(family, "order 0 turns", t, "status", f["status"])
        assert t[0:8].max() < t[8:12].min()
    for f in two_orders(inp.case_chain_blocks(1), family):
        t = f["turns"]
        print(family, "order 1 turns", t, "status", f["status"])
        assert t[4:12].max() < t[0:4].min()


@pytest.mark.parametrize("max_iter", [1, 3])
@pytest.mark.parametrize("family", FAMILIES)
def test_d_every_lambda_uses_up_max_iter(family, max_iter):
    for f in two_orders(inp.case_max_iter(max_iter), family):
        assert set(f["status"]) == {4} and set(f["n_done"]) == {10}
        assert (f["iter"][1:] == max_iter).all(), f["iter"]


@pytest.mark.parametrize("family", FAMILIES)
def test_e_penalty_factors(family):
    case = inp.case_penalty_factors()
    for f in two_orders(case, family):
        assert (f["nb_active"][0] == 2).all(), f["nb_active"][0]
        assert (f["beta"][[3, 17]] != 0).all()
        print(family, "covariate", f["beta"][40], "best", f["best"], "n_done", f["n_done"])
        assert (f["beta"][40] != 0).any()


def test_f_model_saturated():
    for f in two_orders(inp.case_saturated(), "logistic"):
        assert set(f["status"]) == {3}
        print("saturated: n_done", f["n_done"])


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("family", FAMILIES)
def test_g_constant_columns(family, dense):
    case = inp.case_constant_columns(dense)
    X, fold = case["X"], case["fold"]
    for j, c in (inp.G_ZERO_DENSE if dense else inp.G_ZERO_2BIT):
        assert np.ptp(X[fold != c, j]) == 0                     # constant on the chain's training rows
    for j in (7, 8, 9) + ((11, 13) if dense else ()):
        assert np.ptp(X[:, j]) > 0                              # ... while the column as a whole varies
    if dense:
        # what makes lo == hi necessary.  The statement: the row-by-row mean of 0.1 is not 0.1, so ss about it is not 0.
        # The kernel: its tree returns 0.1 exactly on these folds (a build without the line passes on columns 10 and 11),
        # but not 1 / 3, on any fold
        for k in range(3):
            tr = fold != k
            x = X[tr, 10]
            assert ((x - np.cumsum(x)[-1] / x.size) ** 2).sum() > 0
            assert inp.device_tree_sum(np.where(tr, X[:, 10], 0.0)) / tr.sum() == 0.1
            c = inp.device_tree_sum(np.where(tr, X[:, 12], 0.0)) / tr.sum()
            assert c != 1.0 / 3.0 and inp.device_tree_sum(np.where(tr, (X[:, 12] - c) ** 2, 0.0)) > 0
        tr = fold != 0
        assert inp.device_tree_sum(np.where(tr, X[:, 13], 0.0)) / tr.sum() != 1.0 / 3.0
    for f in two_orders(case, family):
        z = np.zeros(f["beta"].shape, dtype=bool)
        for j, c in (inp.G_ZERO_DENSE if dense else inp.G_ZERO_2BIT):
            z[j, c] = True
        assert (f["beta"][z] == 0).all() and (f["beta"][~z] != 0).any()
        assert np.isfinite(f["beta"]).all() and np.isfinite(f["intercept"]).all()


@pytest.mark.parametrize("dense", [False, True])
def test_h_everything_monomorphic(dense):
    for f in two_orders(inp.case_monomorphic(dense), "linear"):
        assert (f["lambda"][:4] == 0).all() and set(f["status"]) == {1} and set(f["n_done"]) == {4} and (f["beta"] == 0).all()


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("n,m", inp.SMALL_SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_i_small_shapes(family, n, m, dense):
    case = inp.case_small(n, m, dense)
    assert np.array_equal(case["X"][:, 0], np.arange(n) % 3)
    for k in range(2):
        yt = case["ys"]["logistic"][case["fold"] != k]
        assert yt.min() == 0 and yt.max() == 1
    for f in two_orders(case, family):
        assert np.isfinite(f["beta"]).all() and (f["status"] > 0).all()


@pytest.mark.parametrize("family", FAMILIES)
def test_j_byte_image_through_a_selection(family):
    k, rows, cols, case = inp.case_byte_selection()
    assert rows.size == 333 and (np.diff(rows) < 0).any() and np.array_equal(cols, np.arange(0, 60, 2))
    assert case["covar"].shape == (333, 2) and case["pf_covar"] is None      # (unpenalised: the default)
    for f in two_orders(case, family):
        assert (f["beta"][30:] != 0).all() and (f["best"] > 0).all()
