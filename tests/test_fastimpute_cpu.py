"""snp_fastImpute without a GPU: the CPU statement (tests/native/fastimpute_ref.cpp over fastimpute_step.hpp, the header the
kernels are compiled from) against a direct numpy definition, the split rule on hand-made columns, the reference's own
expectations (tests/testthat/test-3-fastImpute.R:9-107) on the statement, the header and the statement under a sanitizer
as a stand-alone program, and the host mirror's refusals and predictor lists."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import fastimpute_inputs as fi  # noqa: E402
import fastimpute_ref as ref  # noqa: E402
import impute_ref  # noqa: E402

SEED = fi.SEED


def run(g, preds, p_train=0.8, seed=SEED, **kw):
    off, idx = ref.lists(preds)
    return ref.fast_impute(g, off, idx, p_train, seed, **kw)


# ---- 1. the statement against the direct definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 17, 64, 200])
@pytest.mark.parametrize("npred", [0, 1, 5, 12])
def test_statement_against_the_numpy_definition(n, npred):
    """bytes and infos exactly equal (infos are ratios of integers), first-round trees included; predictors with
    missing calls, a variant without a missing call and one without an observed call among them"""
    m = npred + 4
    g = fi.random_image(n, m, 100 * n + npred, missing=0.15)
    g[:, m - 1] = 3
    g[:, m - 2] = np.minimum(g[:, m - 2], 2) % 3
    preds = [np.array([k for k in range(m) if k != j][:npred], dtype=np.int32) for j in range(m)]
    few = [p if j < 3 or j >= m - 2 else p[:0] for j, p in enumerate(preds)]   # the numpy definition is slow: three full models
    out, infos, n_all, tr = run(g, few, p_train=0.7, trace=True)
    want, want_infos, want_all = fi.numpy_fast_impute(g, few, 0.7, SEED)
    assert np.array_equal(out, want)
    assert np.array_equal(infos, want_infos, equal_nan=True)
    assert n_all == want_all == int((g == 3).all(0).sum()) >= 1
    assert (g[:, few[0]] == 3).any() or npred == 0 or n < 17   # missing predictors are present
    for j in range(m):
        if 0 < (g[:, j] == 3).sum() < n:
            assert fi.trace_splits(tr[j]) == fi.numpy_target(g, j, few[j], 0.7, SEED)[2][0]
    assert np.array_equal(run(g, few, p_train=0.7, nthreads=4)[0], out)


def test_exp_and_log_ports_agree_with_libm():
    rng = np.random.default_rng(3)
    for x in np.r_[rng.uniform(-30, 30, 200), 0.0, -0.0, 1e-300]:
        assert abs(fi.exp_det(x) - np.exp(x)) <= 1e-13 * np.exp(x)
    for x in np.r_[rng.uniform(1e-7, 1.0, 200), 0.5, 1.0, 1e-7]:
        assert abs(fi.log_det(x) - np.log(x)) <= 1e-13 * max(1.0, abs(np.log(x)))


# ---- 2. the split rule on hand-made columns -------------------------------------------------------------------------------------
def _target_with(n=90, seed=4):
    """a target (variant 0) whose calls cycle 0, 1, 2 and whose last nine samples are missing"""
    y = (np.arange(n) % 3).astype(np.uint8)
    col = y.copy()
    col[n - 9:] = 3
    return y, col


def test_a_copy_of_the_target_is_chosen_at_the_root():
    y, col = _target_with()
    noise = np.random.default_rng(1).integers(0, 3, y.size).astype(np.uint8)
    g = np.asfortranarray(np.stack([col, noise, y], axis=1))
    out, infos, _, tr = run(g, [[1, 2], [], []], trace=True)
    root = tr[0, 0]
    # labels 0 | 0.5, 1: the first threshold separates most gradient; no predictor call is missing, so direction 0
    assert list(root) == [1, 0, 0]
    assert tr[0, 1, 0] == -1 and list(tr[0, 2]) == [1, 1, 0]          # left child pure, right child splits 1 | 2 on the copy
    assert list(out[-9:, 0] - 4) == list(y[-9:]) and infos[1, 0] == 0.0


def test_two_identical_predictors_tie_and_the_smaller_position_wins():
    y, col = _target_with()
    g = np.asfortranarray(np.stack([col, y, y], axis=1))
    tr = run(g, [[1, 2], [], []], trace=True)[3]
    assert (tr[0, :, 0] != 1).all() and tr[0, 0, 0] == 0
    swapped = run(g, [[2, 1], [], []], trace=True)
    assert np.array_equal(swapped[3], tr) and np.array_equal(swapped[0], run(g, [[1, 2], [], []])[0])


def test_a_child_below_min_child_weight_is_rejected():
    """h = p (1 - p) <= 1 / 4: a child needs at least four training samples, so a predictor that singles out three is
    no candidate, and one that singles out eight is"""
    n = 40
    col = np.zeros(n, dtype=np.uint8)
    col[:3] = 2
    col[-1] = 3
    few = (np.arange(n) < 3).astype(np.uint8)
    g = np.asfortranarray(np.stack([col, few], axis=1))
    out, _, _, tr = run(g, [[1], []], p_train=1.0, trace=True)
    assert tr[0, 0, 0] == -1 and (tr[0, 1:, 0] == -2).all()
    col[:8] = 2
    g = np.asfortranarray(np.stack([col, (np.arange(n) < 8).astype(np.uint8)], axis=1))
    assert run(g, [[1], []], p_train=1.0, trace=True)[3][0, 0, 0] == 0


@pytest.mark.parametrize("label", [0, 1, 2])
def test_constant_labels_give_a_root_leaf_and_that_call(label):
    n = 50
    col = np.full(n, label, dtype=np.uint8)
    col[::7] = 3
    x = np.random.default_rng(label).integers(0, 4, n).astype(np.uint8)
    out, infos, _, tr = run(np.asfortranarray(np.stack([col, x], axis=1)), [[1], []], trace=True)
    if label != 1:   # base is clamped to 1e-7: gradients of 1e-7 give no gain above 1e-6
        assert tr[0, 0, 0] == -1
    assert (out[::7, 0] == 4 + label).all() and infos[1, 0] == 0.0


def test_a_feature_missing_exactly_where_the_label_is_2_splits_at_2_5_with_missing_right():
    n = 120
    y = (np.arange(n) % 3 == 2).astype(np.uint8) * 2
    col = y.copy()
    col[-12:] = 3
    # calls 0 / 1 / 2 unrelated to the label, missing iff label 2: only t = 2.5 has every call on the left (with calls
    # 0 / 1 alone, t = 1.5 would do the same and win the tie)
    x = np.where(y == 2, 3, (np.arange(n) // 3) % 3).astype(np.uint8)
    _, infos, _, tr = run(np.asfortranarray(np.stack([col, x], axis=1)), [[1], []], trace=True)
    assert list(tr[0, 0]) == [0, 2, 0] and infos[1, 0] == 0.0


def test_an_empty_predictor_list_gives_a_root_leaf():
    g = fi.random_image(60, 2, 9, missing=0.2)
    out, infos, _, tr = run(g, [[], []], trace=True)
    assert (tr[:, 0, 0] == -1).all() and (tr[:, 1:, 0] == -2).all()
    for j in range(2):
        assert np.unique(out[g[:, j] == 3, j]).size == 1   # one margin, one call


def test_sums_of_1e5_quantised_gradients_do_not_depend_on_the_order():
    n = 100000
    g = fi.random_image(n, 4, 21, missing=0.05)
    preds = fi.window_lists(4, 3)
    out, infos, _ = run(g, preds, p_train=1.0, nthreads=4)     # p_train = 1: the roles do not move with the sample index
    perm = np.random.default_rng(5).permutation(n)
    out2, infos2, _ = run(np.asfortranarray(g[perm]), preds, p_train=1.0, nthreads=4)
    assert np.array_equal(out2, out[perm]) and np.array_equal(infos2, infos, equal_nan=True)


# ---- 3. the reference's expectations ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example():
    ex = fi.example_case()
    ex["preds"] = fi.numpy_lists(ex["G"], ex["chr"], ex["ind"])
    ex["out"], ex["infos"], ex["n_all"] = run(ex["G"], ex["preds"], p_train=0.6, nthreads=8)
    return ex


def test_example_data_errors_follow_their_estimate(example):
    """test-3-fastImpute.R:21-64 on the CPU statement with SEED: 100 variants meet the recipe (374.7 predictors on average:
    most fall back to the window).  Measured: F = 5637 on (1, 99) degrees of freedom, p = 4.4e-89 (the reference asks
    for < 2e-16); slope of actual on estimated errors 1.006; 45.3 % errors on the 10 000 masked calls against 51.7 %
    for `mode`.  Seeds 1 and 2 give p = 6e-85 / 1e-86, 44.9 % / 44.5 %."""
    ex = example
    G, G0, ind, out, infos = ex["G"], ex["G0"], ex["ind"], ex["out"], ex["infos"]
    assert ind.size == 100 and (G == 3).sum() == 100 * ind.size
    mask = G[:, ind] == 3
    nb_err = ((out[:, ind] - 4 != G0[:, ind]) & mask).sum(0)
    nb_err_est = infos[0, ind] * infos[1, ind] * ex["n"]
    F, p, slope = fi.f_test_through_origin(nb_err, nb_err_est)
    rate = nb_err.sum() / mask.sum()
    mode = impute_ref.impute(G, "mode")[0]
    mode_rate = ((mode[:, ind] - 4 != G0[:, ind]) & mask).sum() / mask.sum()
    print("F", F, "p", p, "slope", slope, "errors", rate, "mode", mode_rate)
    assert p < 2e-16
    assert nb_err.sum() < ((mode[:, ind] - 4 != G0[:, ind]) & mask).sum()
    # nothing else moved; no missing call remains
    assert np.array_equal(out[G != 3], G[G != 3]) and ex["n_all"] == 0 and out.max() <= 6 and not (out == 3).any()
    assert np.array_equal(infos[0], (G == 3).mean(0)) and np.isnan(infos[1, np.setdiff1d(np.arange(ex["m"]), ind)]).all()


def test_randomness_cannot_be_imputed():
    """test-3-fastImpute.R:68-76: 100 x 200 uniform codes 0 .. 3; measured mean(infos[1]) = 0.671 with SEED"""
    rng = np.random.default_rng(SEED)
    g = np.asfortranarray(rng.integers(0, 4, (100, 200)).astype(np.uint8))
    out, infos, n_all = run(g, fi.window_lists(200, 200))
    print("mean validation error", np.nanmean(infos[1]))
    assert not np.isnan(infos[1]).any() and infos[1].mean() > 0.5
    assert n_all == 0 and not (out == 3).any()


def test_missing_calls_remain_only_where_no_call_is_observed():
    """test-3-fastImpute.R:80-91"""
    rng = np.random.default_rng(SEED + 1)
    g = np.asfortranarray(rng.integers(0, 4, (100, 200)).astype(np.uint8))
    ind = np.arange(150, 161)
    g[:, ind] = 3
    out, infos, n_all = run(g, fi.window_lists(200, 10))
    left = (out == 3).sum(0)
    assert n_all == ind.size and (left[ind] == 100).all() and (np.delete(left, ind) == 0).all()
    assert (infos[0, ind] == 1).all() and np.isnan(infos[1, ind]).all()


def test_same_seed_same_bytes_other_seed_other_bytes():
    """test-3-fastImpute.R:95-105"""
    g = fi.random_image(150, 30, 77, missing=0.2)
    preds = fi.window_lists(30, 6)
    a, b, c = run(g, preds, seed=2), run(g, preds, seed=2, nthreads=2), run(g, preds, seed=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1], equal_nan=True)


# ---- 4. the header and the statement under a sanitizer --------------------------------------------------------------------------
def test_header_under_a_sanitizer(tmp_path):
    exe = str(tmp_path / "fastimpute_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-ffp-contract=off", "-std=c++17",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "bigsnpr_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "native"),
                           os.path.join(ROOT, "tests", "native", "fastimpute_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks held" in out.stdout


# ---- 5. the host mirror without a device ------------------------------------------------------------------------------------------
def _fbm(ba, n=10, m=6, code=None):
    Gna = ba.FBM_code256.__new__(ba.FBM_code256)   # the checks come before the image is looked at
    Gna.code256 = ba.CODE_012.copy() if code is None else code
    Gna._bed = type("Image", (), dict(nrow=n, ncol=m, handle=None))()
    return Gna


def test_argument_errors_need_no_gpu():
    import bigsnpr_amd as ba
    with pytest.raises(ValueError, match="identical.*CODE_012.* is not TRUE"):
        ba.snp_fastImpute(_fbm(ba, code=ba.CODE_IMPUTE_PRED), np.ones(6))
    with pytest.raises(ValueError, match="identical.*CODE_012.* is not TRUE"):
        ba.snp_fastImpute(_fbm(ba, code=ba.CODE_DOSAGE), np.ones(6))
    with pytest.raises(TypeError, match="not of class 'FBM.code256'"):
        ba.snp_fastImpute(np.zeros((3, 3), dtype=np.uint8), np.ones(3))
    with pytest.raises(ValueError, match="^Incompatibility between dimensions\\.$"):
        ba.snp_fastImpute(_fbm(ba), 1)
    for kw, text in ((dict(p_train=0), "p_train"), (dict(p_train=1.5), "p_train"), (dict(alpha=0), "alpha"),
                     (dict(alpha=2), "alpha"), (dict(size=0), "size"), (dict(n_cor=1), "n_cor"), (dict(n_cor=11), "n_cor")):
        with pytest.raises(ValueError, match="'%s' must" % text):
            ba.snp_fastImpute(_fbm(ba), np.ones(6), **kw)


def test_predictor_lists_from_a_sparse_correlation_matrix():
    """both triangles of the upper-triangular slots count; stored zeros and NaN do not; fewer than 5 -> the window,
    clipped at the ends of the chromosome; indices are those of the whole image, ascending"""
    import bigsnpr_amd as ba
    m = 20
    chr1, chr2 = np.arange(0, 12), np.arange(12, 20)
    dense = np.zeros((12, 12))
    for r in (0, 1, 2, 3, 4, 8):
        dense[r, 6] = 0.5          # variant 6 gets 0 .. 4 from above the diagonal ...
    dense[6, 9] = dense[6, 11] = -0.3   # ... and 9, 11 from its row
    dense[8, 6] = 0.0
    up = np.triu(dense, 1)
    p = np.r_[0, np.cumsum((up != 0).sum(0))]
    i = np.concatenate([np.flatnonzero(up[:, c]) for c in range(12)])
    x = np.concatenate([up[np.flatnonzero(up[:, c]), c] for c in range(12)])
    # a stored zero and a stored NaN in column 6
    at = p[7]
    i, x = np.insert(i, at, 5), np.insert(x, at, np.nan)
    p[7:] += 1
    empty = (np.zeros(0, dtype=np.int32), np.zeros(9, dtype=np.int32), np.zeros(0))
    off, idx = ba.predictor_lists(m, [(chr1, i, p, x), (chr2,) + empty], size=3)
    lists = [list(idx[off[j]:off[j + 1]]) for j in range(m)]
    assert lists[6] == [0, 1, 2, 3, 4, 9, 11]            # 5 (NaN) and 8 (zero) are left out
    assert lists[0] == [1, 2, 3] and lists[11] == [8, 9, 10] and lists[5] == [2, 3, 4, 6, 7, 8]   # 6 alone: the window
    assert lists[12] == [13, 14, 15] and lists[19] == [16, 17, 18] and lists[14] == [12, 13, 15, 16, 17]   # never across
    assert off[0] == 0 and off[-1] == idx.size and idx.dtype == np.int32 and off.dtype == np.int64
    # interleaved chromosomes: the window is in variant indices, the members are the chromosome's
    off, idx = ba.predictor_lists(6, [(np.array([0, 2, 4]), *empty[:1], np.zeros(4, dtype=np.int32), empty[2]),
                                      (np.array([1, 3, 5]), *empty[:1], np.zeros(4, dtype=np.int32), empty[2])], size=2)
    assert [list(idx[off[j]:off[j + 1]]) for j in range(6)] == [[2], [3], [0, 4], [1, 5], [2], [3]]
