"""snp_ldsplit without a GPU: the CPU statement (tests/native/ldsplit_ref.cpp) against the reference's published 4 x 4
example, against a brute force over every split of small matrices, and against its own definition on a larger one; the
host mirror's loop over max_size; and the proof that each input of tests/helpers/ldsplit_inputs.py contains what the
device tests use it for."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ldsplit_ref as ref  # noqa: E402

sparse = pytest.importorskip("scipy.sparse")
import ldsplit_inputs as inputs  # noqa: E402

INF = float("inf")
NA = -1


@pytest.fixture(scope="module")
def example():
    """corr[i, j] = (i + j) / 10 (1-based), unit diagonal"""
    A = np.add.outer(np.arange(1, 5) / 10, np.arange(1, 5) / 10)
    np.fill_diagonal(A, 1.0)
    return sparse.csc_matrix(A)


def _levels(A, min_size, max_size, max_K, pos):
    p, i, x = ref.csc(A)
    return ref.split(p, i, x, A.shape[0], 0.0, min_size, max_size, max_K, 1.0, INF, pos)


def test_example_one_to_four(example):
    r = _levels(example, 1, 4, 5, np.zeros(4))
    assert r["best_ind"].T.tolist() == [[4, 4, 4, 4], [1, 2, 3, NA], [1, 2, NA, NA], [1, NA, NA, NA], [NA] * 4]
    want = [[0, 0, 0, 0], [0.5, 0.61, 0.49, INF], [1.11, 1.10, INF, INF], [1.6, INF, INF, INF], [INF] * 4]
    for got, exp in zip(r["C"].T, want):
        fin = np.isfinite(exp)
        assert np.array_equal(np.isfinite(got), fin)
        assert np.allclose(got[fin], np.array(exp)[fin], rtol=0, atol=1e-6)


def test_example_two_blocks_of_two(example):
    r = _levels(example, 2, 2, 3, np.ones(4))
    assert r["best_ind"].T.tolist() == [[NA, NA, 4, NA], [2, NA, NA, NA], [NA] * 4]
    assert r["C"][:, 0].tolist() == [INF, INF, 0, INF]
    assert abs(r["C"][0, 1] - 1.02) <= 1e-6 and np.all(np.isinf(r["C"][1:, 1])) and np.all(np.isinf(r["C"][:, 2]))


def test_example_position_windows(example):
    r = _levels(example, 1, 3, 3, np.linspace(0, 1, 4))
    assert r["best_ind"][:, 0].tolist() == [NA, 4, 4, 4]
    pos = np.arange(1, 5) * 2.0
    assert ref.snp_ldsplit(example, 0, 1, 3, max_K=3, max_r2=1, max_cost=INF, pos_scaled=pos) is None
    res = ref.snp_ldsplit(example, 0, 1, 3, max_K=4, max_r2=1, max_cost=INF, pos_scaled=pos)
    assert len(res["n_block"]) == 1 and res["n_block"][0] == 4
    r = _levels(example, 1, 3, 4, pos)
    assert r["best_ind"].T.tolist() == [[NA, NA, NA, 4], [NA, NA, 3, NA], [NA, 2, NA, NA], [1, NA, NA, NA]]


def test_example_perc_kept_is_exact(example):
    res = ref.snp_ldsplit(example, 0, 1, 2, 4, max_r2=1, max_cost=INF)
    assert res["n_block"].tolist() == [2, 3, 4]
    assert res["perc_kept"].tolist() == [8 / 16, 6 / 16, 4 / 16]


def test_python_transliteration_agrees():
    """the C statement against rules 1 - 5 written out in Python, on small matrices with ties, Inf entries, a position
    window and a finite max_cost"""
    rng = np.random.default_rng(5)
    for trial in range(40):
        m = int(rng.integers(6, 30))
        A = inputs.banded(m, int(rng.integers(1, 6)), 100 + trial, p_zero=float(rng.choice([0.3, 0.7])))
        p, i, x = ref.csc(A)
        mn = int(rng.integers(1, 5))
        mx = int(rng.integers(mn, min(m, mn + 8) + 1))
        kw = dict(thr_r2=float(rng.choice([0, 0.1])), min_size=mn, max_size=mx, max_K=int(rng.integers(1, 12)),
                  max_r2=float(rng.choice([0.1, 1])), max_cost=float(rng.choice([INF, 0.5, 2.0])),
                  pos_scaled=np.sort(rng.uniform(0, 3, m)) if trial % 2 else None)
        r = ref.split(p, i, x, m, **kw)
        C, best, levels = ref.py_split(p, i, x, m, **kw)
        assert np.array_equal(r["C"], C) and np.array_equal(r["best_ind"], best) and r["levels_run"] == levels, (trial, kw)


def _compositions(m, lo, hi):
    if m == 0:
        yield ()
    for s in range(lo, min(hi, m) + 1):
        for rest in _compositions(m - s, lo, hi):
            yield (s,) + rest


@pytest.mark.parametrize("m", range(6, 13))
def test_brute_force(m):
    """Every split of m variants into blocks of allowed sizes.  The entries are dyadic, so the directly summed costs are
    exact and "optimal" is an exact statement; the statement's cost may differ by the float rounding of E (1e-6 relative)."""
    rng = np.random.default_rng(m)
    lo = int(rng.integers(1, 3))
    hi = int(rng.integers(lo + 1, m))
    thr = 0.1 if m % 2 else 0.0
    A = inputs.banded(m, 4, 300 + m, p_zero=0.3, p_half=0.3)
    p, i, x = ref.csc(A)
    r = ref.split(p, i, x, m, thr, lo, hi, m, 1.0, INF)
    best = {}
    for sizes in _compositions(m, lo, hi):
        last = np.cumsum(sizes) - 1
        cost, _ = inputs.outside_cost(A, last, thr)
        key = (cost, float(np.sum(np.square(sizes))))
        K = len(sizes)
        best[K] = min(best.get(K, key), key)
    assert best
    for K in range(1, m + 1):
        if K not in best:
            assert not r["ok"][K - 1] and np.isinf(r["cost"][K - 1])
            continue
        assert r["ok"][K - 1]
        assert abs(r["cost"][K - 1] - best[K][0]) <= 1e-6 * best[K][0]
        assert r["cost2"][K - 1] == best[K][1]
        sizes = np.diff(np.concatenate([[0], r["all_last"][K - 1, :K]]))
        assert sizes.sum() == m and np.all((sizes >= lo) & (sizes <= hi))


@pytest.fixture(scope="module")
def corr400():
    """a seeded 401-variant banded correlation matrix of simulated genotypes (real-valued entries)"""
    m, band = 401, 12
    rng = np.random.default_rng(2024)
    base = rng.binomial(2, 0.3, size=(300, m)).astype(float)
    for j in range(1, m):   # neighbours share alleles
        mix = rng.random(300) < 0.6
        base[mix, j] = base[mix, j - 1]
    R = np.corrcoef(base, rowvar=False)
    R[np.isnan(R)] = 0
    ii, jj = np.indices((m, m))
    R[np.abs(ii - jj) > band] = 0
    np.fill_diagonal(R, 1.0)
    return sparse.csc_matrix(R)


def test_consistency(corr400):
    """A reported cost is a sum of at most K floats (E, each within 2^-24 relative of its fp64 sum) added in fp64: within
    2^-23 relative of the directly summed r^2 outside the blocks."""
    m = corr400.shape[0]
    res = ref.snp_ldsplit(corr400, 0.02, 10, 30, max_K=50, max_r2=1.0, max_cost=INF)
    assert res["n_block"].tolist() == list(range(14, 41))      # ceil(401 / 30) .. floor(401 / 10)
    for row in range(len(res["n_block"])):
        last, size = res["all_last"][row], res["all_size"][row]
        assert last[-1] == m - 1 and np.array_equal(np.diff(np.concatenate([[-1], last])), size)
        assert np.all((size >= 10) & (size <= 30)) and res["cost2"][row] == np.sum(size ** 2)
        direct, _ = inputs.outside_cost(corr400, last, 0.02)
        assert abs(res["cost"][row] - direct) <= 2.0 ** -23 * direct
    lim = ref.snp_ldsplit(corr400, 0.02, 10, 30, max_K=50, max_r2=0.3, max_cost=INF)
    assert lim is not None and np.any(sparse.tril(corr400, k=-1).data ** 2 > 0.3)
    for row in range(len(lim["n_block"])):
        assert inputs.outside_cost(corr400, lim["all_last"][row], 0.02)[1] <= 0.3


def test_several_max_size(corr400):
    """shuffled values of max_size: the single runs in ascending order, a number of blocks reported again only at a
    strictly lower cost"""
    args = dict(max_K=45, max_r2=1.0, max_cost=INF)
    both = ref.snp_ldsplit(corr400, 0.02, 10, [40, 20, 30], **args)
    best, want = {}, []
    for one in (20, 30, 40):
        single = ref.snp_ldsplit(corr400, 0.02, 10, one, **args)
        for row in range(len(single["n_block"])):
            K, cost = int(single["n_block"][row]), float(single["cost"][row])
            if cost < best.get(K, INF):
                best[K] = cost
                want.append((one, K, cost, float(single["cost2"][row]), float(single["perc_kept"][row]),
                             single["all_last"][row].tolist()))
    got = [(int(both["max_size"][r]), int(both["n_block"][r]), float(both["cost"][r]), float(both["cost2"][r]),
            float(both["perc_kept"][r]), both["all_last"][r].tolist()) for r in range(len(both["n_block"]))]
    assert got == want and len({w[0] for w in want}) > 1


def test_inputs_contain_what_they_are_for():
    def counters(name):
        A, kw = inputs.named(name)
        p, i, x = ref.csc(A)
        r = ref.split(p, i, x, A.shape[0], **kw)
        return A, kw, r, r["counters"]

    _, _, _, c = counters("ties")
    assert c["by_cost2"] > 0 and c["full_tie"] > 0
    _, _, _, c = counters("max_r2")
    assert c["best_with_inf"] > 0 and c["finite_levels"] > 0
    _, kw, r, _ = counters("early_stop")
    assert 1 < r["levels_run"] < kw["max_K"]
    _, _, _, c = counters("window")
    assert c["E_window"] > 0 and c["level0_window"] == 1
    A, _, r, _ = counters("diagonal_only")
    assert A.indptr[58] - A.indptr[57] == 1 and A.indices[A.indptr[57]] == 57 and r["ok"].any()
    A, kw, r, _ = counters("thr_r2")
    x2 = sparse.tril(A, k=-1).data ** 2
    assert np.any(x2 < kw["thr_r2"]) and np.any(x2 >= kw["thr_r2"]) and r["ok"].any()
    k = inputs.kernel_constants()
    for name, rest in (("ties", 1), ("max_r2", k["kRowTile"] - 1), ("window", 0)):
        A, kw = inputs.named(name)
        assert A.shape[0] % k["kRowTile"] == rest and kw["max_size"] - kw["min_size"] + 1 > 4 * k["kSplit"]
    _, kw, r, _ = counters("W_is_1")
    assert kw["min_size"] == kw["max_size"] and r["ok"].sum() == 1 and not r["ok"][-1]
    A, kw, r, _ = counters("max_size_is_m")
    assert kw["max_size"] == A.shape[0] and kw["min_size"] == 1 and r["ok"].all()
    _, kw, r, _ = counters("level_0_only")
    assert kw["max_K"] == 1 and r["ok"].tolist() == [1]
    _, kw, r, _ = counters("moderate")
    assert r["ok"].sum() > 10 and r["counters"]["full_tie"] > 0


@pytest.mark.parametrize("name", inputs.NAMES)
def test_gather_in_the_header_s_order_equals_the_sequential_loops(name):
    """what the kernels do per row — the minimum of the candidates in the order of ldsplit_step.hpp, over partial minima
    of the t range — against the reference's replacement rule over col = m - 1 .. 0, on the host"""
    A, kw = inputs.named(name)
    p, i, x = ref.csc(A)
    r = ref.split(p, i, x, A.shape[0], **kw)
    for split in (1, inputs.kernel_constants()["kSplit"]):
        C, best, levels = ref.gather(p, i, x, A.shape[0], split=split, **kw)
        assert np.array_equal(C, r["C"]) and np.array_equal(best, r["best_ind"]) and levels == r["levels_run"]


def test_kernel_constants_are_readable():
    k = inputs.kernel_constants()      # the device tests derive m and W from these
    assert all(k[name] > 0 for name in inputs.CONSTANTS)
