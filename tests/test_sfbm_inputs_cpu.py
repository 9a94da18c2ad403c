"""The inputs of tests/test_gpu_sfbm_shapes.py, tests/test_gpu_ldpred2_auto_shapes.py and tests/test_gpu_chain_batches.py
(tests/helpers/sfbm_inputs.py) without a GPU: each one crosses the threshold
of the loop it is meant for, the thresholds being read from bigsnpr_amd/csrc/sparse_ld.hip, and the references are well
behaved on it (no NaN column, every chain moves, a positive definite system whose iteration bound scipy's MINRES keeps).
If a constant of the kernels is retuned, the test here names the input that no longer covers its loop."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import auto_statement  # noqa: E402
import lassosum2_ref  # noqa: E402
import ldpred2_auto_ref as auto_ref  # noqa: E402
import ldpred2_ref  # noqa: E402
import sfbm_inputs as si  # noqa: E402
from scipy import sparse  # noqa: E402
from scipy.sparse import linalg as sla  # noqa: E402

TOL = 1e-10          # sp_solve_sym's default


@pytest.fixture(scope="module")
def K():
    k = si.kernel_constants()
    assert set(k) == set(si.CONSTANTS) and all(v > 0 for v in k.values())
    return k


@pytest.fixture(scope="module")
def mixed(K):
    A = si.mixed_band()
    return A, si.mixed_subset(A, K["kShortBelow"])


@pytest.fixture(scope="module")
def wide():
    return si.wide_band()


# ---- thresholds ---------------------------------------------------------------------------------------------------------------

def test_mixed_band_is_past_every_stride(K, mixed):
    A, sub = mixed
    m2 = A.shape[0]
    assert (abs(A - A.T)).nnz == 0 and np.all(A.diagonal() == 1)
    assert np.unique(sub).size == sub.size and np.any(np.diff(sub) < 0)
    long_groups = K["kMaxColBlocks"] * K["kBlock"] // 64                  # waves of the long-column launch
    short_groups = K["kMaxColBlocks"] * K["kBlock"] // K["kShortLanes"]    # groups of lanes of the short-column launch
    for name, s in (("whole", None), ("subset", sub)):
        long_, short = si.column_lists(A, s, K["kShortBelow"])
        print("mixed_band %s: %d long columns (a wave takes a second one past %d), %d short (past %d), nnz %d"
              % (name, long_.size, long_groups, short.size, short_groups, A.nnz))
        assert long_.size > long_groups, "mixed_band (%s) no longer strides the long-column launch of k_columns" % name
        assert short.size > short_groups, "mixed_band (%s) no longer strides the short-column launch of k_columns" % name
    # every vector of the solve lives on the columns of corr, also under a subset
    assert m2 > K["kMaxVecBlocks"] * K["kBlock"], "mixed_band no longer strides k_sumsq / k_solve_*"
    # rocprim's radix sort of the off-diagonal entries: several times the 2.3e5 of the bed_cor matrices
    assert sparse.triu(A, k=1).nnz > 5e5


def test_wide_band_needs_a_second_round_and_fits_the_window(K, wide):
    A = wide
    L = np.diff(A.indptr)
    lasso_round = 64 * K["kAxpyBatch"]
    gibbs_round = K["kGibbsThreads"] * K["kGibbsAxpy"]
    print("wide_band: nnz %d, column lengths %d .. %d, %d columns past %d, %d past %d"
          % (A.nnz, L.min(), L.max(), np.sum(L > lasso_round), lasso_round, np.sum(L > gibbs_round), gibbs_round))
    assert np.sum(L > lasso_round) > 100, "wide_band no longer needs a second round in k_lassosum2"
    assert np.sum(L > gibbs_round) > 100, "wide_band no longer needs a second round in k_ldpred2_gibbs"
    fp, fi, _ = si.csc_arrays(A)
    fits, rows = ldpred2_ref.envelope(fp, fi, A.shape[0])
    assert fits and rows <= ldpred2_ref.window_rows(), "wide_band no longer takes the LDS window"
    assert sparse.triu(A, k=1).nnz > 2e6
    # the subsets of the GPU tests: the sorted one keeps the window, the unsorted one takes the general path
    srt, uns = si.wide_subsets(A.shape[0])
    assert ldpred2_ref.envelope(fp, fi, A.shape[0], srt)[0] and not ldpred2_ref.envelope(fp, fi, A.shape[0], uns)[0]
    for sub in (srt, uns):
        assert np.sum(L[sub] > max(lasso_round, gibbs_round)) > 100


# ---- the cells of the pair loads ----------------------------------------------------------------------------------------------------

def test_aligned_columns_hold_every_cell(K):
    short_below = K["kShortBelow"]
    for tail in ("odd", "even"):
        p, i, x, m2, lengths = si.aligned_columns(tail)
        assert p[-1] == i.size == x.size and p[-1] % 2 == (1 if tail == "odd" else 0)
        assert lengths[-1] >= short_below and lengths[0] >= short_below and p[0] == 0          # long last column, long column at 0
        assert np.all(i >= 1) and np.all(i < m2)                                               # row 0 is stored nowhere
        for c in range(m2):
            r = i[p[c]:p[c + 1]]
            assert np.all(np.diff(r) > 0) and np.all(r % 2 == (1 if c % 2 == 0 else 0))        # ascending, of the column's class
        cells = si.alignment_cells(p, lengths, short_below)
        for start in (0, 1):
            for mod in (si.STEP - 1, 0, 1):
                for lpar in (0, 1):
                    if lpar != mod % 2:
                        continue        # the length's parity follows from its remainder: 127 and 1 are odd, 0 is even
                    assert (start, lpar, mod) in cells, (tail, start, lpar, mod)
        # both sides of the boundary between the two kernels, and the other listed lengths, at both start parities
        for L in si.SHORT_SPECIALS + si.LONG_SPECIALS:
            starts = {int(p[c] % 2) for c in range(m2) if lengths[c] == L}
            assert starts == {0, 1}, (tail, L, starts)
        assert short_below - 1 in si.SHORT_SPECIALS and short_below in si.SHORT_SPECIALS
        # a neighbour in memory is of the other class, except next to the empty columns
        v = [si.poisoned_vector(m2, k, 1) for k in (0, 1)]
        for c in range(m2):
            assert np.all(np.abs(v[c % 2][i[p[c]:p[c + 1]]]) < 10) and v[c % 2][0] == si.POISON
            if 0 < p[c] < p[c + 1] and lengths[c - 1] > 0:
                assert v[c % 2][i[p[c] - 1]] == si.POISON
            if p[c] < p[c + 1] < p[-1] and lengths[c + 1] > 0:
                assert v[c % 2][i[p[c + 1]]] == si.POISON


# ---- the solve ----------------------------------------------------------------------------------------------------------------------

def test_gershgorin_and_iteration_bound(mixed):
    A, sub = mixed
    d = si.mixed_shift(A.shape[0])
    b = si.mixed_rhs(A.shape[0])
    for name, M, rhs in (("whole", A + sparse.diags(d), b), ("subset", si.submatrix(A, sub) + sparse.diags(d[sub]), b[sub])):
        M = sparse.csc_matrix(M)
        lo, hi = si.gershgorin(M)
        assert lo > 0
        kappa = hi / lo
        k_tol, k_room = si.minres_iterations(kappa, TOL), si.minres_iterations(kappa, TOL / 100)
        # k(tol) iterations suffice: scipy's MINRES, stopped there (its own stopping rule switched off), is within tol
        seen = []
        x, _ = sla.minres(M, rhs, rtol=1e-300, maxiter=k_tol, callback=lambda xk: seen.append(
            np.linalg.norm(rhs - M @ xk) / np.linalg.norm(rhs)))
        needed = 1 + next(k for k, r in enumerate(seen) if r <= TOL)
        print("mixed_band %s: Gershgorin [%.3f, %.3f], kappa_G %.3f, k(tol) = %d, k(tol / 100) = %d, scipy MINRES reaches tol "
              "after %d iterations" % (name, lo, hi, kappa, k_tol, k_room, needed))
        assert needed <= k_tol < k_room
        x_ref = sla.splu(M).solve(rhs)
        relres_ref = np.linalg.norm(rhs - M @ x_ref) / np.linalg.norm(rhs)
        assert relres_ref < 1e-13


# ---- the statements on wide_band and the small systems ----------------------------------------------------------------------------

def _committed_long(beta, sub, lo=1100, hi=1900):
    """a non-zero beta at a column in [lo, hi): every such column of wide_band has more than 2 048 entries"""
    cols = np.arange(beta.shape[0]) if sub is None else sub
    inside = (cols >= lo) & (cols < hi)
    return np.all(np.any(beta[inside] != 0, axis=0))


def test_wide_band_statements_move_long_columns(K, wide):
    A = wide
    m2 = A.shape[0]
    L = np.diff(A.indptr)
    assert np.all(L[1100:1900] > max(64 * K["kAxpyBatch"], K["kGibbsThreads"] * K["kGibbsAxpy"]))
    fp, fi, fx = si.csc_arrays(A)
    bh = si.wide_beta_hat(m2)
    srt, uns = si.wide_subsets(m2)
    for sub in (None, srt, uns):
        b = bh if sub is None else bh[sub]
        beta, iters, moves, _ = lassosum2_ref.grid(fp, fi, fx, m2, b, np.ones(b.size), si.WIDE_LAMBDA, si.WIDE_DELTA, ind_sub=sub,
                                                   maxiter=si.WIDE_MAXITER, nthreads=16)
        print("lassosum2 on wide_band (%s): moves %s, num_iter %s" % ("whole" if sub is None else "subset", moves, iters))
        assert np.isfinite(beta).all() and np.all(moves > 0) and _committed_long(beta, sub)
    df = si.df_of(bh, si.WIDE_N)
    assert np.max(np.abs(si.gibbs_inputs(df)[1] - bh)) <= 2 ** -52 * np.max(np.abs(bh))
    for sub in (None, uns):
        beta, moves = si.gibbs_statement(ldpred2_ref, A, si.take(df, sub), si.WIDE_CHAINS, 2024, sub=sub, burn_in=si.WIDE_BURN_IN,
                                         num_iter=si.WIDE_NUM_ITER)
        print("Gibbs on wide_band (%s): moves %s" % ("whole" if sub is None else "subset", moves))
        assert np.isfinite(beta).all() and np.all(moves > 0) and _committed_long(beta, sub)
    smp, moves = ldpred2_ref.sampling(fp, fi, fx, m2, bh, np.full(m2, si.WIDE_N), 0.2, 0.05, 0, stream=3, burn_in=si.WIDE_BURN_IN,
                                      num_iter=si.WIDE_NUM_ITER, seed=2024)
    assert moves > 0 and np.any(smp[1100:1900, -1] != 0)


@pytest.mark.parametrize("m", si.SMALL_M)
def test_small_statements_move(m):
    E = si.small_with_empty_columns()
    L = np.diff(E.indptr)
    assert E.shape == (si.SMALL_M2, si.SMALL_M2) and L[si.EMPTY] == 0 and L[si.EMPTY_WITH_DIAGONAL] == 1
    assert E[si.EMPTY_WITH_DIAGONAL, si.EMPTY_WITH_DIAGONAL] == 1 and ((E != 0) != (E != 0).T).nnz == 0
    for name, A, sub, df in si.small_cases(m):
        assert df["beta"].size == m and (sub is None or sub.size == m)
        if sub is not None and m >= 2:
            assert si.EMPTY in sub and si.EMPTY_WITH_DIAGONAL in sub
            assert np.all(np.diff(sub) > 0) == (name == "ascending")
        beta, iters, spars, moves = si.lassosum2_statement(lassosum2_ref, A, df, sub=sub, **si.SMALL_LASSO)
        assert beta.shape == (m, 8) and np.isfinite(beta).all() and np.all(moves > 0), (m, name, moves)
        beta, moves = si.gibbs_statement(ldpred2_ref, A, df, si.SMALL_CHAINS, 77, sub=sub, burn_in=si.SMALL_BURN_IN,
                                         num_iter=si.SMALL_NUM_ITER)
        assert beta.shape == (m, 3) and np.isfinite(beta).all() and np.all(moves > 0), (m, name, moves)


# ---- LDpred2-auto: the statement alone on the inputs of tests/test_gpu_ldpred2_auto_shapes.py ----------------------------------------

def _auto(A, df, sub, kw, seed=si.AUTO_SEED):
    """the statement with the mean LD score summed on the host: (list of chains, raw output with path_nb and moves)"""
    return auto_statement.expected(si.full_of(A), df, auto_statement.host_mean_ld(A, sub), seed=seed, sub=sub, **kw)


def _finite(want):
    return all(np.isfinite(w[k]).all() for w in want for k in auto_statement.ARRAYS + auto_statement.SCALARS)


def test_wide_band_auto_needs_a_second_round_and_wraps_the_ring(K, wide):
    A = wide
    m2 = A.shape[0]
    L = np.diff(A.indptr)
    gibbs_round = K["kGibbsThreads"] * K["kGibbsAxpy"]
    assert L.max() > gibbs_round, "wide_band no longer needs a second round of add_column in k_ldpred2_auto"
    fp, fi, _ = si.csc_arrays(A)
    for name, sub, df, ascending in si.wide_auto_cases(A):
        fits, rows = auto_ref.envelope(fp, fi, m2, sub)
        assert fits == ascending, name
        if ascending:
            # fewer ring rows than rows of dotprods: the ring wraps, a row r is not at ring[r]
            assert rows <= auto_ref.window_rows() and rows < m2, (name, rows)
        assert np.sum((L if sub is None else L[sub]) > gibbs_round) > 100, name
        want, raw = _auto(A, df, sub, si.AUTO_WIDE)
        print("auto on wide_band (%s): envelope %d rows, moves %s" % (name, rows, raw["moves"]))
        assert _finite(want) and np.all(raw["moves"] > 0) and np.all(raw["path_nb"] >= 0), name
        assert all(w["sample_beta"].shape == (df["beta"].size, 3) for w in want)


@pytest.mark.parametrize("m", si.SMALL_M)
def test_small_auto_statements_move(m):
    block = 64
    for name, A, sub, df in si.small_cases(m):
        want, raw = _auto(A, df, sub, si.AUTO_SMALL)
        nb = raw["path_nb"]
        print("auto on %d coordinates (%s): moves %s, causal %d .. %d" % (m, name, raw["moves"], nb.min(), nb.max()))
        assert _finite(want) and np.all(raw["moves"] > 0) and np.all(nb >= 0) and np.all(nb <= m), (m, name)
        if m >= block - 1:
            # the append to ind_causal starts inside the first block of 64 positions and, where m allows, behind it
            below, at_or_above = np.any(nb < block, axis=0), np.any(nb >= block, axis=0)
            assert np.any(below & at_or_above) if m >= block else below.any(), (m, name, nb.min(axis=0), nb.max(axis=0))
        if m <= 2:
            assert np.any((nb >= 1) & (nb <= 2))          # the MLE on one or two causal variants


def test_straddle_case_ends_sweeps_on_both_sides_of_one_stride(K):
    A, df = si.straddle_case()
    stride = K["kGibbsThreads"]
    want, raw = _auto(A, df, None, si.STRADDLE)
    nb = raw["path_nb"][:, 0]
    print("straddle: %d sweeps below %d, %d at it, %d above, range %d .. %d"
          % (np.sum(nb < stride), stride, np.sum(nb == stride), np.sum(nb > stride), nb.min(), nb.max()))
    assert _finite(want) and raw["moves"][0] > 0 and nb.min() >= 0
    assert np.any(nb < stride) and np.any(nb == stride) and np.any(nb > stride)
    assert np.all(want[0]["path_p_est"] == si.STRADDLE["p_bounds"][0])


def test_window_limit_matrices_sit_on_both_sides_of_the_largest_window():
    W = auto_ref.window_rows()
    seen = []
    for half, fits, A, df in si.window_limit_cases(W):
        fp, fi, _ = si.csc_arrays(A)
        got_fits, rows = auto_ref.envelope(fp, fi, A.shape[0])
        assert A.shape[0] == si.WINDOW_LIMIT_M2 and rows == 2 * half + 64
        assert got_fits == fits, (half, rows)
        if fits:
            assert -(-rows // 64) * 64 == W, "the fitting matrix no longer asks for the largest window"
        else:
            assert rows > W
        seen.append(fits)
    assert seen == [True, False]


def test_batch_inputs_move_every_chain_and_grid_point():
    """the inputs of tests/test_gpu_chain_batches.py: the visiting order differs from the given one, the stream ids are
    not the positions, and no chain or grid point stands still (a stale buffer would then change nothing)"""
    gp = si.BATCH_CHAINS
    assert gp["p"].size == 5 and np.unique(gp["p"]).size == 5 and np.any(np.diff(gp["p"]) > 0)          # not large p first
    assert not np.array_equal(gp["stream"], np.arange(5)) and np.array_equal(gp["p"], si.BATCH_AUTO["vec_p_init"])
    assert max(si.BATCH_CAPS) < 5 and 5 % 2 and 5 % 4 and 8 % 3 and 3 in si.BATCH_CAPS_LASSO          # a shorter last batch
    kw = {k: v for k, v in si.BATCH_AUTO.items() if k != "stream"}
    for name, A, sub, df in si.batch_cases():
        assert df["beta"].size == (si.SMALL_M2 if sub is None else si.BATCH_M)
        assert sub is None or (si.EMPTY in sub and si.EMPTY_WITH_DIAGONAL in sub)
        beta, iters, spars, moves = si.lassosum2_statement(lassosum2_ref, A, df, sub=sub, **si.SMALL_LASSO)
        assert beta.shape[1] == 8 and np.isfinite(beta).all() and np.all(moves > 0), (name, moves)
        beta, moves = si.gibbs_statement(ldpred2_ref, A, df, gp, 77, sub=sub, burn_in=si.SMALL_BURN_IN, num_iter=si.SMALL_NUM_ITER)
        assert np.isfinite(beta).all() and np.all(moves > 0), (name, moves)
        assert np.unique(beta, axis=1).shape[1] == 5
        want, raw = _auto(A, df, sub, dict(kw, stream=si.BATCH_AUTO["stream"]), seed=77)
        assert _finite(want) and np.all(raw["moves"] > 0), (name, raw["moves"])


def test_repeated_index_statement_equals_the_transliteration():
    from bigsnpr_amd.lassosum2 import lassosum2_inputs
    A = si.small_with_empty_columns()
    ind = si.repeated_subset()
    assert ind.size == 200 and ind.min() >= 0 and ind.max() < si.SMALL_M2
    assert ind[3] == ind[9] and ind[20] == ind[21] and ind[190] == ind[191]                 # inside one block of 64 positions
    assert np.intersect1d(ind[:64], ind[128:]).size > 0 and np.unique(ind).size < ind.size        # across blocks
    df = si.small_df(200, 700)
    fp, fi, fx = si.csc_arrays(A)
    scale, bh, pf, lam, dl = lassosum2_inputs(df["beta"], df["beta_se"], df["n_eff"], si.SMALL_LASSO["delta"],
                                              si.SMALL_LASSO["nlambda"], 0.01)
    beta, iters, moves, _ = lassosum2_ref.grid(fp, fi, fx, si.SMALL_M2, bh, pf, lam, dl, ind_sub=ind,
                                               maxiter=si.SMALL_LASSO["maxiter"], nthreads=2)
    print("repeated ind_corr: moves %s, num_iter %s, NaN columns %s" % (moves, iters, np.isnan(beta).all(axis=0)))
    assert np.all(moves > 0) and np.isfinite(beta).all(axis=0).sum() >= lam.size // 2
    for g in range(lam.size):
        pb, pk = lassosum2_ref.py_one(fp, fi, fx, si.SMALL_M2, bh, pf * lam[g], pf * dl[g] + 1, ind, 200e3,
                                      si.SMALL_LASSO["maxiter"], 1e-5)
        assert np.array_equal(beta[:, g], pb, equal_nan=True), g
        assert iters[g] == pk, (g, iters[g], pk)
    want, it2, _, _ = si.lassosum2_statement(lassosum2_ref, A, df, sub=ind, **si.SMALL_LASSO)
    assert np.array_equal(want, beta * scale[:, None], equal_nan=True) and np.array_equal(it2, iters)
