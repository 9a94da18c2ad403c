"""knn_parallel / prob_dist / LOF on the device (bigsnpr_amd/csrc/knn.hip) against the CPU statement compiled from the same
knn_step.hpp (tests/native/knn_ref.cpp): indices, distances and both statistics bit for bit, for every slab count.
tests/test_knn_cpu.py holds that statement to plain NumPy."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import knn_cases as cases  # noqa: E402
import knn_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def basic():
    X = cases.scores(1000, 20, 7)
    return X, ref.knn(X, None, 6)


@pytest.fixture(scope="module")
def planted():
    X = cases.planted_outliers()
    return X, ref.prob_dist(X, 5), ref.lof(X, (4, 10, 30))


def same_table(got, want):
    assert got["nn_idx"].dtype == np.int32 and got["nn_idx"].flags.f_contiguous
    assert np.array_equal(got["nn_idx"], want["nn_idx"])
    assert np.array_equal(got["nn_dists"], want["nn_dists"])


def slabs(monkeypatch, s):
    if s is None:
        monkeypatch.delenv("BSN_KNN_SLABS", raising=False)
    else:
        monkeypatch.setenv("BSN_KNN_SLABS", str(s))


def test_basic(ba, basic, monkeypatch):
    slabs(monkeypatch, None)
    X, want = basic
    got = ba.knn_parallel(X, k=6)
    same_table(got, want)
    st = ba.knn_last_stats()
    # the planner's own S: 4 query blocks of 256, no slab shorter than 128 points (for any device of 25 CUs or more)
    assert st["slabs"] == ref.plan(1000, 1000, 6, forced=0)["S"] == 7
    assert st["query_block"] == 256


def test_merge_path_ragged_slabs(ba, basic, monkeypatch):
    X, want = basic
    slabs(monkeypatch, 1)
    one = ba.knn_parallel(X, k=6)
    assert ba.knn_last_stats()["slabs"] == 1
    slabs(monkeypatch, 7)                        # 1000 / 7: ragged
    got = ba.knn_parallel(X, k=6)
    assert ba.knn_last_stats()["slabs"] == 7
    same_table(got, want)
    same_table(got, one)
    slabs(monkeypatch, 0)                        # below 1: the planner's rule
    same_table(ba.knn_parallel(X, k=6), want)


@pytest.mark.parametrize("S", [1, 5])
def test_ties_on_a_grid_of_duplicates(ba, monkeypatch, S):
    X = cases.grid_ties()
    want = ref.knn(X, None, 31)
    slabs(monkeypatch, S)
    got = ba.knn_parallel(X, k=31)
    assert ba.knn_last_stats()["slabs"] == S
    same_table(got, want)
    assert not (got["nn_idx"] == np.arange(600)[:, None]).any()          # the own index is absent ...
    assert (got["nn_dists"][:, :3] == 0).all()                           # ... the duplicates are present
    assert (X[got["nn_idx"][:, 0]] == X).all()


@pytest.mark.parametrize("n,p,k", [(300, 1, 1), (300, 5, 64), (200, 64, 1), (150, 64, 64), (65, 5, 64), (2, 1, 1), (33, 61, 32)])
def test_edges_of_p_and_k(ba, monkeypatch, n, p, k):
    X = cases.scores(n, p, 100 + n)
    want = ref.knn(X, None, k)
    for S in (None, 3):
        slabs(monkeypatch, S)
        same_table(ba.knn_parallel(X, k=k), want)
    if k == n - 1:                                # every other point is a neighbour
        assert (np.sort(want["nn_idx"], axis=1) == np.array([np.delete(np.arange(n), i) for i in range(n)])).all()


def test_query_mode(ba, monkeypatch):
    X = cases.scores(777, 20, 8)
    Q = cases.scores(130, 20, 9) * np.sqrt(130 / 777)
    rows = [5, 400, 776]
    Q[[0, 64, 129]] = X[rows]
    want = ref.knn(X, Q, 9)
    for S in (None, 4):
        slabs(monkeypatch, S)
        got = ba.knn_parallel(X, Q, k=9)
        same_table(got, want)
        assert got["nn_idx"].shape == (130, 9)
        assert list(got["nn_idx"][[0, 64, 129], 0]) == rows and (got["nn_dists"][[0, 64, 129], 0] == 0).all()
    # k = n is allowed here: nothing is left out
    same_table(ba.knn_parallel(X[:40], Q, k=40), ref.knn(X[:40], Q, 40))


def test_several_blocks_partial_tiles(ba, monkeypatch):
    slabs(monkeypatch, None)
    X = cases.scores(2500, 20, 10)
    want = ref.knn(X, None, 31)
    got = ba.knn_parallel(X, k=31)
    same_table(got, want)
    assert ba.knn_last_stats()["query_block"] == 128      # 20 blocks, the last one partial; 2500 = 78 tiles of 32 + 4


@pytest.mark.parametrize("S", [1, 3])
def test_statistics_on_planted_outliers(ba, planted, monkeypatch, S):
    X, pd_ref, lof_ref = planted
    n = X.shape[0]
    slabs(monkeypatch, S)
    pd = ba.prob_dist(X, kNN=5)
    assert ba.knn_last_stats()["slabs"] == S
    assert np.array_equal(pd["dist_self"], pd_ref["dist_self"])
    assert np.array_equal(pd["dist_nn"], pd_ref["dist_nn"])
    assert np.array_equal(pd["S"], pd_ref["dist_self"] / np.sqrt(pd_ref["dist_nn"]))
    M = ba.lof_matrix(X, (4, 10, 30))
    assert np.array_equal(M, lof_ref)
    planted_set = set(range(n - cases.PLANTED, n))
    assert set(np.argsort(pd["S"])[-cases.PLANTED:]) == planted_set
    lof = ba.LOF(X)
    assert np.array_equal(lof, np.log(lof_ref.max(axis=1)))
    assert set(np.argsort(lof)[-cases.PLANTED:]) == planted_set
    assert np.array_equal(ba.LOF(X, seq_k=(4, 10), combine=np.mean, log=False), lof_ref[:, :2].mean(axis=1))


def test_duplicates_give_inf_and_nan(ba, monkeypatch):
    slabs(monkeypatch, None)
    X = np.repeat(cases.lattice(8, 2, 3, seed=0), 6, axis=0)
    with np.errstate(all="ignore"):
        want = ref.lof(X, (4,))
    got = ba.lof_matrix(X, (4,))
    assert np.isnan(got).all() and np.array_equal(np.isnan(got), np.isnan(want))


def test_end_to_end_on_example_bed(ba, monkeypatch):
    slabs(monkeypatch, None)
    obj = ba.bed(os.path.join(GOLDEN, "example.bed"))
    svd = ba.bed_autoSVD(obj, k=10, verbose=False)
    u = np.asarray(svd["u"])
    assert u.shape[1] == 10
    pd = ba.prob_dist(u)
    want = ref.prob_dist(u, 5)
    assert np.array_equal(pd["dist_self"], want["dist_self"])
    assert np.array_equal(pd["dist_nn"], want["dist_nn"])
    assert np.isfinite(pd["S"]).all() and (pd["S"] > 0).all()


def test_two_calls_return_the_same_bytes(ba, basic, monkeypatch):
    X, _ = basic
    for S in (None, 7):
        slabs(monkeypatch, S)
        a, b = ba.knn_parallel(X, k=6), ba.knn_parallel(X, k=6)
        assert a["nn_idx"].tobytes() == b["nn_idx"].tobytes() and a["nn_dists"].tobytes() == b["nn_dists"].tobytes()
        p, q = ba.prob_dist(X), ba.prob_dist(X)
        assert p["dist_self"].tobytes() == q["dist_self"].tobytes() and p["dist_nn"].tobytes() == q["dist_nn"].tobytes()
        assert ba.lof_matrix(X).tobytes() == ba.lof_matrix(X).tobytes()


def raw_knn(ba, X, Q, k, p=None):
    """bsn_knn itself, past the mirror's own checks: the return code and the library's message"""
    from bigsnpr_amd import _lib
    L = _lib.load()
    n = X.shape[0]
    nq = n if Q is None else Q.shape[0]
    p = X.shape[1] if p is None else p
    kk = max(1, min(k, 128))
    idx, dist = np.zeros((nq, kk), dtype=np.int32, order="F"), np.zeros((nq, kk), order="F")
    dX = _lib.DeviceArray.from_numpy(X)
    dQ = None if Q is None else _lib.DeviceArray.from_numpy(Q)
    try:
        rc = L.bsn_knn(dX.ptr, n, n, None if dQ is None else dQ.ptr, nq, nq, p, k, idx.ctypes.data_as(_lib.i32p),
                       dist.ctypes.data_as(_lib.f64p))
        return rc, L.bsn_last_error().decode() if rc else ""
    finally:
        dX.free()
        if dQ is not None:
            dQ.free()


def test_refusals_by_name_leave_the_library_usable(ba, basic, monkeypatch):
    slabs(monkeypatch, None)
    X, want = basic
    small = cases.scores(30, 4, 1)

    def usable():
        same_table(ba.knn_parallel(X, k=6), want)

    rc, msg = raw_knn(ba, small, None, 30)                         # k = n in self mode
    assert rc != 0 and "'k' should be at most 29" in msg, msg
    usable()
    rc, msg = raw_knn(ba, cases.scores(100, 4, 1), None, 65)
    assert rc != 0 and "'k' should be in range [1, 64]" in msg, msg
    rc, msg = raw_knn(ba, small, None, 0)
    assert rc != 0 and "'k' should be in range [1, 64]" in msg, msg
    usable()
    rc, msg = raw_knn(ba, cases.scores(100, 65, 1), None, 3)
    assert rc != 0 and "should be in range [1, 64] (got 65)" in msg and "'p'" in msg, msg
    rc, msg = raw_knn(ba, small, None, 3, p=0)
    assert rc != 0 and "'p'" in msg, msg
    usable()
    for bad in (np.nan, np.inf, -np.inf):
        Y = small.copy()
        Y[17, 2] = bad
        rc, msg = raw_knn(ba, Y, None, 3)
        assert rc != 0 and "non-finite value" in msg and "'data'" in msg, msg
        with pytest.raises(ba.BsnError, match="non-finite value"):
            ba.prob_dist(Y)
        with pytest.raises(ba.BsnError, match="non-finite value"):
            ba.LOF(Y, seq_k=(3,))
        usable()
    Qb = small[:7].copy()
    Qb[6, 3] = np.nan
    rc, msg = raw_knn(ba, small, Qb, 3)
    assert rc != 0 and "non-finite value" in msg and "'query'" in msg, msg
    usable()
    # the mirror refuses the same before a device is asked
    with pytest.raises(ValueError, match="'k' should be at most 29"):
        ba.knn_parallel(small, k=30)


def test_rob_maha(ba, monkeypatch):
    slabs(monkeypatch, None)
    X = cases.planted_outliers()
    A = np.random.default_rng(3).normal(size=(10, 10))
    X = X @ A                                                    # correlated columns of unequal scale
    Ut = ba.rob_maha(X)
    assert np.array_equal(Ut, ba.rob_maha(X))                    # the transform itself is reproducible
    pd = ba.prob_dist(X, robMaha=True)
    want = ref.prob_dist(Ut, 5)
    assert np.array_equal(pd["dist_self"], want["dist_self"])
    assert np.array_equal(pd["dist_nn"], want["dist_nn"])
    assert np.array_equal(ba.lof_matrix(X, (4, 10), robMaha=True), ref.lof(Ut, (4, 10)))
    n = X.shape[0]
    assert set(np.argsort(pd["S"])[-cases.PLANTED:]) == set(range(n - cases.PLANTED, n))
