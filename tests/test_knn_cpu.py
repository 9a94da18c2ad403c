"""knn_parallel / prob_dist / LOF without a device: the CPU statement (tests/native/knn_ref.cpp over
bigsnpr_amd/csrc/knn_step.hpp — the header the kernels use) against plain NumPy, the planner of knn_plan.hpp, and the
argument checks of the mirror.  tests/test_gpu_knn.py holds the device to this statement bit for bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import knn_cases as cases  # noqa: E402
import knn_ref as ref  # noqa: E402


# ---- the order: exact arithmetic, many ties ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,side,k", [(300, 3, 4, 31), (257, 1, 9, 5), (200, 6, 2, 64)])
def test_twin_equals_numpy_on_a_lattice_self_mode(n, p, side, k):
    X = cases.lattice(n, p, side, seed=n + p)
    assert np.unique(X, axis=0).shape[0] < n        # duplicated rows exist
    got = ref.knn(X, None, k)
    idx, d2 = cases.np_knn(X, None, k)
    assert np.array_equal(got["nn_idx"], idx)
    assert np.array_equal(got["nn_d2"], d2)
    assert np.array_equal(got["nn_dists"], np.sqrt(d2))
    assert not (got["nn_idx"] == np.arange(n)[:, None]).any()            # the own index is out ...
    assert (got["nn_d2"][:, 0] == 0).sum() > n // 4                     # ... its duplicates are in, at distance 0


def test_twin_equals_numpy_on_a_lattice_query_mode():
    X = cases.lattice(400, 3, 5, seed=1)
    Q = np.concatenate([cases.lattice(57, 3, 5, seed=2), X[[3, 77, 399]]])
    got = ref.knn(X, Q, 12)
    idx, d2 = cases.np_knn(X, Q, 12)
    assert np.array_equal(got["nn_idx"], idx)
    assert np.array_equal(got["nn_dists"], np.sqrt(d2))
    assert (got["nn_dists"][-3:, 0] == 0).all()      # a query copied from the data finds that row: nothing is left out


def test_grid_of_duplicates_ties_across_the_kth_place():
    X = cases.grid_ties()
    got = ref.knn(X, None, 31)
    idx, d2 = cases.np_knn(X, None, 31)
    assert np.array_equal(got["nn_idx"], idx)
    # the k-th and the first left-out candidate are at the same distance for most queries: only the index decides
    full = np.sort(cases.np_d2(X) + np.diag(np.full(600, np.inf)), axis=1)
    assert (full[:, 30] == full[:, 31]).mean() > 0.5


# ---- random doubles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,k,seed", [(500, 20, 10, 1), (400, 5, 30, 2), (300, 64, 7, 3)])
def test_twin_equals_numpy_on_random_doubles(n, p, k, seed):
    X = cases.scores(n, p, seed)
    rtol = 2 * (p + 2) * 2.0 ** -53           # each side within (p + 2) half-ulps of the exact sum
    full = cases.np_d2(X)
    idx, d2 = cases.np_knn(X, None, k, d2=full)
    # rows whose listed or boundary squared distances lie within the bound of each other: the order would not be
    # NumPy's to decide.  The seeds are chosen so that there is none.
    srt = np.sort(full + np.diag(np.full(n, np.inf)), axis=1)[:, :k + 1]
    close = (np.diff(srt, axis=1) <= rtol * srt[:, 1:]).any(axis=1).sum()
    print("rows with squared distances within %.1e of each other: %d" % (rtol, close))
    assert close == 0
    got = ref.knn(X, None, k)
    assert np.array_equal(got["nn_idx"], idx)
    np.testing.assert_allclose(got["nn_d2"], d2, rtol=rtol, atol=0)
    assert np.array_equal(got["nn_dists"], np.sqrt(got["nn_d2"]))


def test_rows_subset_of_the_twin():
    X = cases.scores(300, 20, 4)
    full, part = ref.knn(X, None, 5), ref.knn(X, None, 5, rows=(100, 164))
    assert np.array_equal(full["nn_idx"][100:164], part["nn_idx"][100:164])
    assert np.array_equal(full["nn_dists"][100:164], part["nn_dists"][100:164])


# ---- the statistics -------------------------------------------------------------------------------------------------------
def test_prob_dist_and_lof_equal_their_numpy_transcription_and_find_the_planted_points():
    X = cases.planted_outliers()
    n = X.shape[0]
    seq_k = (4, 10, 30)
    t = ref.knn(X, None, 30)
    pd = ref.prob_dist(X, 5)
    ds, dn = cases.np_prob_dist(t["nn_idx"][:, :5], t["nn_d2"][:, :5])
    np.testing.assert_allclose(pd["dist_self"], ds, rtol=1e-13, atol=0)
    np.testing.assert_allclose(pd["dist_nn"], dn, rtol=1e-13, atol=0)
    lof = ref.lof(X, seq_k)
    np.testing.assert_allclose(lof, cases.np_lof(t["nn_idx"], t["nn_dists"], seq_k), rtol=1e-13, atol=0)
    planted = set(range(n - cases.PLANTED, n))
    S = pd["dist_self"] / np.sqrt(pd["dist_nn"])
    assert set(np.argsort(S)[-cases.PLANTED:]) == planted
    assert set(np.argsort(lof.max(axis=1))[-cases.PLANTED:]) == planted


def test_duplicates_give_inf_and_nan_as_ieee_has_them():
    X = np.repeat(cases.lattice(8, 2, 3, seed=0), 6, axis=0)     # every row six times: all 4-distances are 0
    with np.errstate(all="ignore"):
        lof = ref.lof(X, (4,))
    assert np.isnan(lof).all()                                    # (inf + ...) / 4 / inf


# ---- the planner --------------------------------------------------------------------------------------------------------
def test_plan_one_slab_when_the_query_blocks_cover_the_cus():
    P = ref.plan(400000, 400000, 5, ncu=256)
    assert (P["qb"], P["nqb"], P["S"], P["partial_bytes"]) == (256, 1563, 1, 0)
    assert ref.plan(100000, 256 * 128, 30, ncu=256)["S"] == 1    # exactly 256 blocks of 128


def test_plan_query_block_follows_the_lds():
    assert [ref.plan(1000, 1000, k)["qb"] for k in (1, 16, 17, 32, 33, 64)] == [256, 256, 128, 128, 64, 64]
    for k in (16, 32, 64):
        assert ref.plan(1000, 1000, k)["qb"] * k * 12 + 32 * 64 * 8 <= 64 * 1024


@pytest.mark.parametrize("n,nq,k,forced", [(400000, 1000, 30, 0), (1000, 1000, 6, 0), (1000, 1000, 6, 7), (600, 600, 31, 5),
                                           (2500, 130, 64, 0), (100, 100, 3, 1000), (65, 65, 64, 0)])
def test_plan_slabs_cover_the_data(n, nq, k, forced):
    P = ref.plan(n, nq, k, ncu=256, forced=forced)
    lo = P["lo"]
    assert lo[0] == 0 and lo[-1] == n and (np.diff(lo) >= 1).all()          # all of 0 .. n, no overlap, none empty
    assert P["S"] <= n
    assert P["partial_bytes"] <= ref.load().knn_partial_cap()
    if forced >= 1:
        assert P["S"] == min(forced, n)
    elif P["S"] > 1:
        assert np.diff(lo).min() >= ref.load().knn_min_slab_points()


def test_plan_small_query_set_is_cut_into_slabs():
    P = ref.plan(400000, 1000, 30, ncu=256)           # 8 blocks of 128 queries
    assert P["nqb"] == 8 and P["S"] == 32 and P["nqb"] * P["S"] >= 256
    assert ref.plan(1000, 1000, 6, ncu=256)["S"] == 7  # 4 blocks; no slab shorter than 128 points


def test_plan_byte_cap_and_clamps():
    cap = ref.load().knn_partial_cap()
    P = ref.plan(2000000, 60000, 64, ncu=256, forced=500)     # 500 slabs would be 23 GB of partial lists
    assert 1 <= P["S"] < 500 and P["partial_bytes"] <= cap < 60000 * (P["S"] + 1) * 64 * 12
    assert ref.plan(50, 50, 3, forced=1000)["S"] == 50         # a forced count above n is clamped
    assert ref.plan(1000, 1000, 6, forced=0)["S"] == ref.plan(1000, 1000, 6, forced=-3)["S"]
    assert [ref.load().knn_padded_p(p) for p in (1, 4, 5, 20, 61, 64)] == [4, 4, 8, 20, 64, 64]


# ---- the mirror's argument checks (no device is touched) -------------------------------------------------------------------
def test_mirror_argument_checks():
    import bigsnpr_amd as ba
    X = cases.scores(20, 3, 0)
    with pytest.raises(TypeError, match="'k' is missing"):
        ba.knn_parallel(X)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.knn_parallel(X, X[:, :2], k=2)
    with pytest.raises(ValueError, match=r"'k' should be at most 19"):
        ba.knn_parallel(X, k=20)                       # self mode: n - 1 candidates
    with pytest.raises(ValueError, match=r"'k' should be in range \[1, 64\]"):
        ba.knn_parallel(X, k=0)
    with pytest.raises(ValueError, match=r"'k' should be in range \[1, 64\]"):
        ba.knn_parallel(cases.scores(100, 3, 0), k=65)
    with pytest.raises(ValueError, match="'k' should be an integer"):
        ba.knn_parallel(X, k=2.5)
    with pytest.raises(ValueError, match="at most 64 columns"):
        ba.prob_dist(np.zeros((100, 65)))
    with pytest.raises(ValueError, match=r"'kNN' should be at most 19"):
        ba.prob_dist(X, kNN=20)
    with pytest.raises(ValueError, match=r"'seq_k' should be at most 19"):
        ba.LOF(X, seq_k=(4, 30))
    with pytest.raises(ValueError, match="'seq_k' should be a non-empty vector"):
        ba.LOF(X, seq_k=())
    with pytest.raises(ValueError, match="should be a matrix"):
        ba.knn_parallel(np.zeros((2, 2, 2)), k=1)
