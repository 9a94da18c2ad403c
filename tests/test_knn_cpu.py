"""knn_parallel / prob_dist / LOF without a device: the CPU statement (tests/native/knn_ref.cpp over
bigsnpr_amd/csrc/knn_step.hpp — the header the kernels use) against plain NumPy, the planner of knn_plan.hpp, and the
argument checks of the mirror.  tests/test_gpu_knn.py holds the device to this statement bit for bit.  The sweep of
tests/knn_cases.py over the scan kernels is held here to the `case` lines of knn.hip (every compiled k_knn_scan<P, QL> has
a shape) and the statement to NumPy at every P of it; tests/test_gpu_knn_shapes.py runs that sweep on the device."""
import os
import re
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


# ---- the sweep over the scan kernels (tests/knn_cases.py) ------------------------------------------------------------------
def compiled_scans():
    """the (P, QL) of the `case P: return k_knn_scan<P, QL>;` lines of scan_of() in knn.hip"""
    with open(os.path.join(ROOT, "bigsnpr_amd", "csrc", "knn.hip")) as f:
        src = f.read()
    found = re.findall(r"case\s+(\d+)\s*:\s*return\s+k_knn_scan<\s*(\d+)\s*,\s*(\d+)\s*>\s*;", src)
    assert found and all(a == b for a, b, _ in found), found
    pairs = [(int(P), int(QL)) for _, P, QL in found]
    assert len(set(pairs)) == len(pairs) == len(re.findall(r"return\s+k_knn_scan<", src)), pairs      # no line missed
    return src, set(pairs)


def test_sweep_reaches_every_compiled_scan_kernel():
    src, compiled = compiled_scans()
    reached = {}
    for p, k, S in cases.sweep():
        P, qb, QL = cases.instantiation(p, k)
        reached.setdefault((P, QL), []).append((p, k, S))
    assert set(reached) == compiled, (sorted(compiled - set(reached)), sorted(set(reached) - compiled))
    assert len(compiled) == 24
    for shapes in reached.values():                                  # each with and without padding, on both slab counts
        assert {P - p for P, p in ((cases.instantiation(p, k)[0], p) for p, k, S in shapes)} == {0, 3}
        assert {S for p, k, S in shapes} == set(cases.SWEEP_S)
    # both sides of the unroll switch U = (P * QL <= 32 ? 4 : 2)
    assert re.search(r"constexpr int U = P \* QL <= 32 \? 4 : 2;", src)
    assert {(16, 2), (32, 1), (36, 1)} <= compiled


def test_sweep_helper_restates_the_header_and_the_dispatch():
    src, _ = compiled_scans()
    # cases.instantiation's QL is knn.hip's rule as it stands today
    assert re.search(r"int queries_per_lane\(int P, int qb\) \{ return P <= 32 && qb >= 256 \? 2 : 1; \}", src)
    L = ref.load()
    for p in range(1, 65):
        for k in range(1, 65):
            P, qb, QL = cases.instantiation(p, k)
            assert P == L.knn_padded_p(p) and qb == ref.plan(1000, 1000, k)["qb"] and qb in (64, 128, 256)
            assert QL == (2 if P <= 32 and qb >= 256 else 1)
    # the geometry the sweep's sizes are chosen for
    n = cases.SWEEP_N
    assert [ref.plan(n, n, k)["nqb"] for k in cases.SWEEP_K] == [3, 5] and n - 2 * 256 == 1
    assert list(np.diff(ref.plan(n, n, 5, forced=3)["lo"])) == [171, 171, 171] and 171 % 32 == 11 and n % 32 == 1


@pytest.mark.parametrize("P", cases.SWEEP_P)
def test_twin_equals_numpy_across_the_sweep(P):
    n = cases.SWEEP_N
    for p in (P - 3, P):
        X = cases.lattice(n, p, 4, seed=p)
        full = cases.np_d2(X)
        for k in cases.SWEEP_K:
            got = ref.knn(X, None, k)
            idx, d2 = cases.np_knn(X, None, k, d2=full)
            assert np.array_equal(got["nn_idx"], idx), (p, k)
            assert np.array_equal(got["nn_d2"], d2), (p, k)
            assert np.array_equal(got["nn_dists"], np.sqrt(d2)), (p, k)
            if P in cases.SWEEP_QUERY_P:
                qb = cases.instantiation(p, k)[1]
                rows, Q = cases.queries_with_copies(X, 2 * qb + 1, p + 100, lambda m, pp, s: cases.lattice(m, pp, 4, s))
                got = ref.knn(X, Q, k)
                idx, d2 = cases.np_knn(X, Q, k)
                assert np.array_equal(got["nn_idx"], idx), (p, k)
                assert np.array_equal(got["nn_d2"], d2), (p, k)
                assert (got["nn_d2"][[0, qb, 2 * qb], 0] == 0).all()


# ---- +inf squared distances from finite coordinates ------------------------------------------------------------------------
def check_huge_table(got, idx, d2, n, k):
    """got (the statement's or the device's table) equals NumPy's (idx, d2) where some squared distances are +inf"""
    assert np.array_equal(got["nn_idx"], idx)
    assert np.array_equal(got["nn_dists"], np.sqrt(d2))
    assert (got["nn_idx"] < n).all() and (got["nn_idx"] >= 0).all()       # a candidate at +inf comes before an unfilled place
    inf = np.isinf(got["nn_dists"])
    assert inf.any() and not np.isnan(got["nn_dists"]).any()
    assert (inf[:, :-1] <= inf[:, 1:]).all()                               # the candidates at +inf come last ...
    both = inf[:, :-1] & inf[:, 1:]
    assert both.any() and (np.diff(got["nn_idx"].astype(np.int64), axis=1)[both] > 0).all()      # ... in order of index


@pytest.mark.parametrize("k", [5, 64])
def test_infinite_squared_distances_order_like_any_value(k):
    n = 70
    X, Q = cases.with_huge(n, 5, seed=3)
    assert np.isfinite(X).all() and np.isfinite(Q).all()
    with np.errstate(over="ignore"):
        full, fullq = cases.np_d2(X), cases.np_d2(X, Q)
    assert not np.isnan(full).any() and np.isinf(full).any() and np.isinf(fullq[-2:]).all()
    got = ref.knn(X, None, k)
    idx, d2 = cases.np_knn(X, None, k, d2=full)
    assert np.array_equal(got["nn_d2"], d2)
    check_huge_table(got, idx, d2, n, k)
    for kq in (k, n):                                    # k = n: every data point is listed, those at +inf included
        got = ref.knn(X, Q, kq)
        idx, d2 = cases.np_knn(X, Q, kq, d2=fullq)
        assert np.array_equal(got["nn_d2"], d2)
        check_huge_table(got, idx, d2, n, kq)
        assert np.array_equal(got["nn_idx"][-2:], np.tile(np.arange(kq, dtype=np.int32), (2, 1)))     # all at +inf: by index
    assert (np.sort(got["nn_idx"], axis=1) == np.arange(n)).all()


# ---- leading dimensions above the row counts -------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [10, 33])
def test_leading_dimension_above_the_row_count(p):
    X, Q = cases.scores(150, p, 5), cases.scores(41, p, 6)
    for q, k in ((None, 7), (Q, 7), (Q, 150)):
        want = ref.knn(X, q, k)
        got = ref.knn(X, q, k, ld=150 + 7, ldq=None if q is None else 41 + 3)     # the rows below hold NaN
        for name in ("nn_idx", "nn_d2", "nn_dists"):
            assert np.array_equal(got[name], want[name]), name
        assert np.isfinite(got["nn_d2"]).all()


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
