"""The kernels of bigsnpr_amd/csrc/sparse_ld.hip where their loops take a second turn: the column stride of k_columns, the
element stride of the solver's vector kernels, the second round of the column update in k_lassosum2 and k_ldpred2_gibbs
(both paths), every cell of the pair loads of k_columns<., 64>, systems of fewer coordinates than one block of 64, repeated
indices in snp_lassosum2, and the upper-triangle expansion at a large sort.  The inputs are synthetic and seeded
(tests/helpers/sfbm_inputs.py); tests/test_sfbm_inputs_cpu.py proves without a GPU, against the constants read from the
source, that each of them crosses its threshold.

References.  Products and LD scores: the summation bound derived in tests/test_gpu_sfbm_products.py, against rational
arithmetic and against scipy.  lassosum2 and the Gibbs sampler: the CPU statements under tests/native, bit for bit.  The
solve: its own residual recomputed in fp64, scipy's sparse LU, and an iteration bound from the Gershgorin interval."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import lassosum2_ref  # noqa: E402
import ldpred2_ref  # noqa: E402
import sfbm_inputs as si  # noqa: E402
from scipy import sparse  # noqa: E402
from scipy.sparse import linalg as sla  # noqa: E402
from sfbm_inputs import check_exact, check_residual, check_scipy  # noqa: E402

TOL = 1e-10          # sp_solve_sym's default


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def K():
    return si.kernel_constants()


@pytest.fixture(scope="module")
def mixed(ba, K):
    A = si.mixed_band()
    sub = si.mixed_subset(A, K["kShortBelow"])
    with ba.as_SFBM(A) as sf:
        yield A, sub, si.submatrix(A, sub), sf


@pytest.fixture(scope="module")
def wide(ba):
    A = si.wide_band()
    with ba.as_SFBM(A) as sf:
        yield A, sf


def _sample(A, sub, K, k=150, seed=1):
    """k random positions, the first and the last, and the positions on both sides of the place in each of the two column
    lists from which a wave (a group of lanes) of k_columns serves its second column"""
    long_, short = si.column_lists(A, sub, K["kShortBelow"])
    g_long = K["kMaxColBlocks"] * K["kBlock"] // 64
    g_short = K["kMaxColBlocks"] * K["kBlock"] // K["kShortLanes"]
    m = long_.size + short.size
    forced = [0, m - 1, long_[g_long - 1], long_[g_long], long_[-1], short[g_short - 1], short[g_short], short[-1]]
    return np.unique(np.concatenate([forced, np.random.default_rng(seed).choice(m, k, replace=False)]))


# ---- 1. products and LD scores past the column stride -------------------------------------------------------------------------------

def test_products_and_ld_scores_past_the_column_stride(ba, K, mixed):
    A, sub, As, sf = mixed
    m2 = A.shape[0]
    rng = np.random.default_rng(3)
    x = rng.normal(size=m2)
    y = ba.sp_prodVec(sf, x)
    check_scipy(A, x, y)
    worst = check_exact(A, x, y, _sample(A, None, K))
    print("sp_prodVec, whole: worst error / ((L + 1) u |A||x|) = %.3f" % worst)
    assert np.array_equal(ba.sp_prodVec(sf, x), y)
    xs = rng.normal(size=sub.size)
    ys = ba.sp_prodVec(sf, xs, ind_corr=sub)
    check_scipy(As, xs, ys)
    worst = check_exact(As, xs, ys, _sample(A, sub, K))
    print("sp_prodVec, subset: worst error / bound = %.3f" % worst)
    assert np.array_equal(ba.sp_prodVec(sf, xs, ind_corr=sub), ys)

    ld = ba.ld_scores_sfbm(sf)
    check_scipy(A, None, ld, square=True)
    worst = check_exact(A, None, ld, _sample(A, None, K), square=True)
    print("ld_scores_sfbm, whole: worst error / bound = %.3f" % worst)
    assert np.array_equal(ba.ld_scores_sfbm(sf), ld)
    lds = ba.ld_scores_sfbm(sf, sub)
    check_scipy(As, None, lds, square=True)
    worst = check_exact(As, None, lds, _sample(A, sub, K), square=True)
    print("ld_scores_sfbm, subset: worst error / bound = %.3f" % worst)
    assert np.array_equal(ba.ld_scores_sfbm(sf, sub), lds)
    # a repeated index gives repeated values (the list is a mask), here with both lists past their strides
    picks = rng.integers(0, sub.size, 30_000)
    perm = rng.permutation(sub.size + picks.size)
    rep = np.concatenate([sub, sub[picks]])[perm]
    long_, short = si.column_lists(A, rep, K["kShortBelow"])
    assert long_.size > K["kMaxColBlocks"] * K["kBlock"] // 64 and short.size > K["kMaxColBlocks"] * K["kBlock"] // K["kShortLanes"]
    got = ba.ld_scores_sfbm(sf, rep)
    assert np.array_equal(got, np.concatenate([lds, lds[picks]])[perm])


# ---- 2. upper form versus full form at the large sort -------------------------------------------------------------------------------

def test_upper_form_equals_full_form_at_the_large_sort(ba, mixed, wide):
    rng = np.random.default_rng(4)
    for name, A, sf in (("mixed_band", mixed[0], mixed[3]), ("wide_band",) + wide):
        m2 = A.shape[0]
        up = sparse.csc_matrix(sparse.triu(A))
        print("%s: %d off-diagonal entries to sort" % (name, up.nnz - m2))
        x = rng.normal(size=m2)
        sub = rng.permutation(m2)[:m2 // 2]
        with ba.as_SFBM(up) as su:
            assert (su.ncol, su.nnz, su.bandwidth) == (sf.ncol, sf.nnz, sf.bandwidth)
            assert su.nnz == A.nnz and su.ncol == m2
            assert np.array_equal(ba.sp_prodVec(su, x), ba.sp_prodVec(sf, x))
            assert np.array_equal(ba.ld_scores_sfbm(su), ba.ld_scores_sfbm(sf))
            assert np.array_equal(ba.sp_prodVec(su, x[:sub.size], ind_corr=sub), ba.sp_prodVec(sf, x[:sub.size], ind_corr=sub))
            assert np.array_equal(ba.ld_scores_sfbm(su, sub), ba.ld_scores_sfbm(sf, sub))
        col = np.repeat(np.arange(m2), np.diff(A.indptr))
        assert sf.bandwidth == np.max(np.abs(col - A.indices))


# ---- 3. MINRES past both strides ------------------------------------------------------------------------------------------------------

def test_solve_past_both_strides(ba, K, mixed):
    """(a) the residual recomputed on the host against the device's (check_residual); (b) against scipy's sparse LU:
    x - x_ref = (A + D)^-1 (r_ref - r_gpu), and ||(A + D)^-1|| ||A + D|| is at most the Gershgorin ratio kappa_G, so
    ||x - x_ref|| / ||x_ref|| <= kappa_G (relres_device + relres_ref); (c) the iteration count.  Wrong block partials would
    spoil alfa, and the restart from the true residual could still drag the solve to tol, so (a) and (b) alone can hide
    them.  For a positive definite system k(t) = ceil(ln(2 / t) / ln((sqrt(kappa) + 1) / (sqrt(kappa) - 1))) iterations
    suffice for a relative residual t (si.minres_iterations); the device gets k(tol / 100): the two digits are the room for
    one restart from the true residual."""
    A, sub, As, sf = mixed
    m2 = A.shape[0]
    assert m2 > K["kMaxVecBlocks"] * K["kBlock"]
    d, b = si.mixed_shift(m2), si.mixed_rhs(m2)
    for name, M, ind in (("whole", A, None), ("subset", As, sub)):
        bb, dd = (b, d) if ind is None else (b[ind], d[ind])
        lo, hi = si.gershgorin(M + sparse.diags(dd))
        assert lo > 0
        kappa = hi / lo
        k_tol, k_room = si.minres_iterations(kappa, TOL), si.minres_iterations(kappa, TOL / 100)
        # (maxiter: a solve that a defect keeps from converging ends with the library's error, not after 10 n iterations)
        sol = ba.sp_solve_sym(sf, bb, add_to_diag=dd, ind_corr=ind, maxiter=10 * k_room)
        assert sol.iters >= 1 and sol.relres <= TOL
        Md, _ = check_residual(M, bb, dd, sol)                                        # (a)
        x_ref = sla.splu(Md).solve(bb)                                                # (b)
        relres_ref = np.linalg.norm(bb - Md @ x_ref) / np.linalg.norm(bb)
        err = np.linalg.norm(np.asarray(sol) - x_ref) / np.linalg.norm(x_ref)
        print("%s: kappa_G %.3f, relres LU %.3e, ||x - x_ref|| / ||x_ref|| = %.3e (allowed %.3e); device iterations %d, "
              "k(tol) = %d, k(tol / 100) = %d" % (name, kappa, relres_ref, err, kappa * (sol.relres + relres_ref), sol.iters,
                                                  k_tol, k_room))
        assert err <= kappa * (sol.relres + relres_ref)
        assert sol.iters <= k_room                                                    # (c)
        again = ba.sp_solve_sym(sf, bb, add_to_diag=dd, ind_corr=ind, maxiter=10 * k_room)
        assert np.array_equal(np.asarray(again), np.asarray(sol)) and again.iters == sol.iters and again.relres == sol.relres


# ---- 4. the cells of the pair loads ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", ["odd", "even"])
def test_alignment_cells(ba, tail):
    """Every column against rationals.  The vector holds 1e300 on row 0 and on the rows of each column's neighbours in
    memory (si.aligned_columns): a half of a pair that is wrongly kept breaks the bound by hundreds of orders, not by an
    ulp.  One vector per class of columns (even and odd index); the columns of the other class see the large values in
    their own terms and are not looked at under that vector."""
    p, i, x, m2, lengths = si.aligned_columns(tail)
    A = sparse.csc_matrix((x, i, p), shape=(m2, m2))
    rng = np.random.default_rng(5)
    half = np.concatenate([[0, m2 - 1], rng.choice(np.arange(1, m2 - 1), m2 // 2 - 2, replace=False)])
    sub = rng.permutation(half)
    As = si.submatrix(A, sub)
    with ba.SFBM(p, i, x, m2, False) as sf, np.errstate(all="ignore"):
        assert sf.nnz == p[-1] and sf.nnz % 2 == (1 if tail == "odd" else 0)
        for klass in (0, 1):
            v = si.poisoned_vector(m2, klass, 6 + klass)
            y = ba.sp_prodVec(sf, v)
            worst = check_exact(A, v, y, np.arange(klass, m2, 2))
            ys = ba.sp_prodVec(sf, v[sub], ind_corr=sub)
            worst_sub = check_exact(As, v[sub], ys, np.nonzero(sub % 2 == klass)[0])
            print("tail %s, columns of class %d: worst error / bound = %.3f whole, %.3f on the subset" % (tail, klass, worst, worst_sub))
        ld = ba.ld_scores_sfbm(sf)
        check_scipy(A, None, ld, square=True)
        worst = check_exact(A, None, ld, np.arange(m2), square=True)
        lds = ba.ld_scores_sfbm(sf, sub)
        check_scipy(As, None, lds, square=True)
        worst_sub = check_exact(As, None, lds, np.arange(sub.size), square=True)
        print("tail %s, LD scores: worst error / bound = %.3f whole, %.3f on the subset" % (tail, worst, worst_sub))


# ---- 5. k_lassosum2, second round of the column update --------------------------------------------------------------------------------

def _device_lassosum2(sf, bh, pf, lam, dl, sub, maxiter, dfmax=200e3, tol=1e-5):
    """bsn_lassosum2 as snp_lassosum2 calls it, on a grid given point by point: (beta [m x G], num_iter [G])"""
    from bigsnpr_amd import _lib
    from bigsnpr_amd._lib import as_f64, check, f64p, i32p, i64p, ptr
    bh, pf, lam, dl = (as_f64(a) for a in (bh, pf, lam, dl))
    sub = None if sub is None else np.ascontiguousarray(sub, dtype=np.int64)
    m, G = bh.size, lam.size
    beta = np.empty((m, G), dtype=np.float64, order="F")
    num_iter = np.zeros(G, dtype=np.int32)
    secs = np.zeros(G)
    check(_lib.load().bsn_lassosum2(sf.handle, ptr(bh, f64p), m, ptr(pf, f64p), ptr(lam, f64p), ptr(dl, f64p), G, ptr(sub, i64p),
                                    float(dfmax), int(maxiter), float(tol), beta.ctypes.data_as(f64p),
                                    num_iter.ctypes.data_as(i32p), secs.ctypes.data_as(f64p)))
    return beta, num_iter


def test_lassosum2_second_round(ba, K, wide):
    from bigsnpr_amd.lassosum2 import _col_means_zero
    A, sf = wide
    m2 = A.shape[0]
    assert np.diff(A.indptr).max() > 64 * K["kAxpyBatch"]
    fp, fi, fx = si.csc_arrays(A)
    bh = si.wide_beta_hat(m2)
    srt, uns = si.wide_subsets(m2)
    for sub in (None, srt, uns):
        b = bh if sub is None else bh[sub]
        pf = np.ones(b.size)
        want, iters, moves, _ = lassosum2_ref.grid(fp, fi, fx, m2, b, pf, si.WIDE_LAMBDA, si.WIDE_DELTA, ind_sub=sub,
                                                   maxiter=si.WIDE_MAXITER, nthreads=16)
        got, num_iter = _device_lassosum2(sf, b, pf, si.WIDE_LAMBDA, si.WIDE_DELTA, sub, si.WIDE_MAXITER)
        assert np.array_equal(got, want, equal_nan=True)
        assert np.array_equal(num_iter, iters)
        assert np.array_equal(_col_means_zero(got), _col_means_zero(want), equal_nan=True)
        assert np.all(moves > 0) and np.isfinite(want).all()


# ---- 6. k_ldpred2_gibbs, second round of the column update, both paths ----------------------------------------------------------------

def test_gibbs_second_round_on_both_paths(ba, K, wide, monkeypatch):
    A, sf = wide
    m2 = A.shape[0]
    assert np.diff(A.indptr).max() > K["kGibbsThreads"] * K["kGibbsAxpy"]
    fp, fi, fx = si.csc_arrays(A)
    fits, rows = ldpred2_ref.envelope(fp, fi, m2)
    assert fits and rows <= ldpred2_ref.window_rows()              # by default this call takes the LDS window
    df = si.df_of(si.wide_beta_hat(m2), si.WIDE_N)
    kw = {"burn_in": si.WIDE_BURN_IN, "num_iter": si.WIDE_NUM_ITER}
    one = {"p": [0.05], "h2": [0.2], "sparse": [False], "stream": [3]}
    want, moves = si.gibbs_statement(ldpred2_ref, A, df, si.WIDE_CHAINS, 2024, **kw)
    assert np.all(moves > 0) and np.isfinite(want).all()
    scale, bh, n = si.gibbs_inputs(df)
    want_smp, _ = ldpred2_ref.sampling(fp, fi, fx, m2, bh, n, 0.2, 0.05, 0, stream=3, seed=2024, **kw)
    win = ba.snp_ldpred2_grid(sf, df, si.WIDE_CHAINS, seed=2024, **kw)
    smp_win = ba.snp_ldpred2_grid(sf, df, one, seed=2024, return_sampling_betas=True, **kw)
    monkeypatch.setenv("BSN_GIBBS_NO_WINDOW", "1")
    gen = ba.snp_ldpred2_grid(sf, df, si.WIDE_CHAINS, seed=2024, **kw)
    smp_gen = ba.snp_ldpred2_grid(sf, df, one, seed=2024, return_sampling_betas=True, **kw)
    monkeypatch.delenv("BSN_GIBBS_NO_WINDOW")
    assert np.array_equal(np.asarray(win), want, equal_nan=True)
    assert np.array_equal(np.asarray(gen), want, equal_nan=True)
    assert np.array_equal(np.asarray(win), np.asarray(gen), equal_nan=True)
    assert np.array_equal(np.asarray(smp_win), want_smp * scale[:, None])
    assert np.array_equal(np.asarray(smp_gen), want_smp * scale[:, None])
    # an unsorted subset: the general path by the host rule
    _, uns = si.wide_subsets(m2)
    assert not ldpred2_ref.envelope(fp, fi, m2, uns)[0]
    dsub = si.take(df, uns)
    want, moves = si.gibbs_statement(ldpred2_ref, A, dsub, si.WIDE_CHAINS, 2024, sub=uns, **kw)
    assert np.all(moves > 0)
    res = ba.snp_ldpred2_grid(sf, dsub, si.WIDE_CHAINS, ind_corr=uns, seed=2024, **kw)
    assert np.array_equal(np.asarray(res), want, equal_nan=True)


# ---- 7. fewer coordinates than a block of 64, one block, just above ---------------------------------------------------------------------

@pytest.mark.parametrize("m", si.SMALL_M)
def test_small_systems(ba, m, monkeypatch):
    kw = {"burn_in": si.SMALL_BURN_IN, "num_iter": si.SMALL_NUM_ITER}
    for name, A, sub, df in si.small_cases(m):
        with ba.as_SFBM(A) as sf:
            assert sf.ncol == (m if sub is None else si.SMALL_M2)
            beta, iters, spars, _ = si.lassosum2_statement(lassosum2_ref, A, df, sub=sub, **si.SMALL_LASSO)
            res = ba.snp_lassosum2(sf, df, ind_corr=sub, **si.SMALL_LASSO)
            assert res.shape == beta.shape == (m, 8), name
            assert np.array_equal(np.asarray(res), beta, equal_nan=True), name
            assert np.array_equal(res.grid_param["num_iter"], iters), name
            assert np.array_equal(res.grid_param["sparsity"], spars, equal_nan=True), name
            want, _ = si.gibbs_statement(ldpred2_ref, A, df, si.SMALL_CHAINS, 77, sub=sub, **kw)
            res = ba.snp_ldpred2_grid(sf, df, si.SMALL_CHAINS, ind_corr=sub, seed=77, **kw)
            assert res.shape == want.shape == (m, 3), name
            assert np.array_equal(np.asarray(res), want, equal_nan=True), name
            if name != "shuffled":          # the ascending orders take the window by default: the general path as well
                fp, fi, _ = si.csc_arrays(A)
                assert ldpred2_ref.envelope(fp, fi, A.shape[0], sub)[0]
                monkeypatch.setenv("BSN_GIBBS_NO_WINDOW", "1")
                gen = ba.snp_ldpred2_grid(sf, df, si.SMALL_CHAINS, ind_corr=sub, seed=77, **kw)
                monkeypatch.delenv("BSN_GIBBS_NO_WINDOW")
                assert np.array_equal(np.asarray(gen), want, equal_nan=True), name


# ---- 8. repeated indices ------------------------------------------------------------------------------------------------------------------

def test_repeated_indices(ba):
    """snp_lassosum2 takes a repeated ind_corr (the reference only asks ind.corr %in% cols_along(corr)); the sampler, the
    product and the solve refuse it before any device work, in the host mirror and in the library"""
    from bigsnpr_amd import _lib
    from bigsnpr_amd._lib import f64p, i32p, i64p, ptr, u64p
    A = si.small_with_empty_columns()
    ind = si.repeated_subset()
    df = si.small_df(ind.size, 700)
    beta, iters, spars, moves = si.lassosum2_statement(lassosum2_ref, A, df, sub=ind, **si.SMALL_LASSO)
    assert np.all(moves > 0)
    x = np.random.default_rng(8).normal(size=ind.size)
    with ba.as_SFBM(A) as sf:
        res = ba.snp_lassosum2(sf, df, ind_corr=ind, **si.SMALL_LASSO)
        assert np.array_equal(np.asarray(res), beta, equal_nan=True)
        assert np.array_equal(res.grid_param["num_iter"], iters)
        assert np.array_equal(res.grid_param["sparsity"], spars, equal_nan=True)
        with pytest.raises(ValueError, match="'ind.corr' should not have repeated indices."):
            ba.snp_ldpred2_grid(sf, df, si.SMALL_CHAINS, ind_corr=ind)
        with pytest.raises(ValueError, match="'ind.corr' should not have repeated indices."):
            ba.sp_prodVec(sf, x, ind_corr=ind)
        with pytest.raises(ValueError, match="'ind.corr' should not have repeated indices."):
            ba.sp_solve_sym(sf, x, add_to_diag=1.0, ind_corr=ind)
        # the library's own refusal, behind the mirror's
        L = _lib.load()
        out = np.full(ind.size * 3, 7.0)
        ones, n_vec = np.ones(ind.size), np.full(ind.size, 1500.0)
        h2, pp, sp, st = np.full(3, 0.3), np.array([1.0, 0.1, 0.01]), np.zeros(3, dtype=np.int32), np.arange(3, dtype=np.uint64)
        it, rr = C.c_int32(0), C.c_double(0.0)
        calls = (lambda: L.bsn_sfbm_prodvec(sf.handle, ptr(x, f64p), ptr(ind, i64p), ind.size, ptr(out, f64p)),
                 lambda: L.bsn_sfbm_solve_sym(sf.handle, ptr(x, f64p), ptr(ones, f64p), ptr(ind, i64p), ind.size, 1e-10, 100,
                                              ptr(out, f64p), C.byref(it), C.byref(rr)),
                 lambda: L.bsn_ldpred2_gibbs(sf.handle, ptr(x, f64p), ptr(n_vec, f64p), ind.size, ptr(ind, i64p), ptr(h2, f64p),
                                             ptr(pp, f64p), ptr(sp, i32p), ptr(st, u64p), 3, 5, 10, 1, ptr(out, f64p), None))
        for call in calls:
            with pytest.raises(ba.BsnError, match="'ind_sub' has [0-9]+ more than once."):
                _lib.check(call())
            assert np.all(out == 7.0)
        # the handle works on
        assert np.array_equal(np.asarray(ba.snp_lassosum2(sf, df, ind_corr=ind, **si.SMALL_LASSO)), np.asarray(res), equal_nan=True)
