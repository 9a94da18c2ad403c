"""Synthetic, seeded inputs for the sparse-LD kernels of bigsnpr_amd/csrc/sparse_ld.hip, sized so that the loops of those
kernels take a second turn, and the checks that the product tests share.  tests/test_sfbm_inputs_cpu.py proves without a
GPU that each input crosses the threshold it is meant for (the thresholds are read from the source, `kernel_constants`);
tests/test_gpu_sfbm_shapes.py runs the device on them, tests/test_gpu_ldpred2_auto_shapes.py runs snp_ldpred2_auto on them
and on the inputs that only its kernel needs, and tests/test_gpu_chain_batches.py the batch loops of the three chain drivers.

The bound of every product check.  A computed sum of L products, in ANY order and with or without fused multiply-adds,
satisfies |fl(sum_k a_k x_k) - sum_k a_k x_k| <= gamma_L sum_k |a_k| |x_k| with gamma_L = L u / (1 - L u) and u = 2^-53
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1), and gamma_L <= (L + 1) u for every L below
9e7: the derivation is in the docstring of tests/test_gpu_sfbm_products.py."""
import math
import os
import re
from fractions import Fraction

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SPARSE_LD = os.path.join(ROOT, "bigsnpr_amd", "csrc", "sparse_ld.hip")

U = 2.0 ** -53
UQ = Fraction(1, 2 ** 53)

POISON = 1e300


# ---- the checks of the product tests ------------------------------------------------------------------------------------------

def exact_column(A, j, x, square=False):
    """(sum, sum of absolute values, number of terms) of column j's terms a_ij x_i (a_ij^2 when `square`), in rationals"""
    lo, hi = A.indptr[j], A.indptr[j + 1]
    s, sa = Fraction(0), Fraction(0)
    for r, a in zip(A.indices[lo:hi], A.data[lo:hi]):
        t = Fraction(float(a)) * (Fraction(float(a)) if square else Fraction(float(x[r])))
        s += t
        sa += abs(t)
    return s, sa, int(hi - lo)


def check_exact(A, x, y, cols, square=False):
    """the bound of the module docstring, in rationals, for the listed columns of A (x: the vector seen by those columns)"""
    worst = 0.0
    for j in cols:
        s, sa, L = exact_column(A, j, x, square)
        err, bound = abs(Fraction(float(y[j])) - s), (L + 1) * UQ * sa
        if sa:
            worst = max(worst, float(err / (UQ * sa)) / (L + 1))
        assert err <= bound, (j, L, float(err), float(bound))
    return worst


def check_scipy(A, x, y, square=False):
    """twice the bound, against scipy's fp64 product, for every column"""
    L = np.diff(A.indptr)
    if square:
        ref = mag = np.asarray(A.multiply(A).sum(axis=0)).ravel()
    else:
        ref, mag = A.T @ x, abs(A).T @ np.abs(x)
    assert np.all(np.abs(y - ref) <= 2 * (L + 1) * U * mag), np.max(np.abs(y - ref) / np.maximum(mag, 1e-300))


def check_residual(A, b, d, sol):
    """the residual of (A + diag(d)) x = b recomputed here in fp64 against the device's.  Both this and the device's
    t = (A + D) x obey the product bound with one term more (the diagonal shift): e_j = (L_j + 2) u (|A + D| |x|)_j each;
    b - t adds u |r_j| each, and a norm of n terms (n + 2) u relative.  So
    | ||r_host|| - ||r_gpu|| | <= 2 ||e + u |r| || + (n + 2) u (||r_host|| + ||r_gpu||).  Returns (A + D, relres_host)."""
    n = b.size
    x = np.asarray(sol)
    Md = sparse.csc_matrix(A + sparse.diags(d))
    r = b - Md @ x
    relres_host = np.linalg.norm(r) / np.linalg.norm(b)
    e = (np.diff(A.indptr) + 2) * U * (abs(Md) @ np.abs(x)) + U * np.abs(r)
    slack = 2 * np.linalg.norm(e) / np.linalg.norm(b) + (n + 2) * U * (relres_host + sol.relres)
    print("iters %d, relres device %.3e host %.3e (allowed difference %.3e)" % (sol.iters, sol.relres, relres_host, slack))
    assert abs(relres_host - sol.relres) <= slack
    return Md, relres_host


# ---- the thresholds, from the source ------------------------------------------------------------------------------------------

CONSTANTS = ("kShortBelow", "kShortLanes", "kBlock", "kMaxColBlocks", "kMaxVecBlocks", "kAxpyBatch", "kGibbsThreads",
             "kGibbsAxpy")


def kernel_constants():
    """the `constexpr` integers of sparse_ld.hip that decide when a loop of its kernels goes round again"""
    with open(SPARSE_LD) as f:
        src = f.read()
    out = {}
    for name in CONSTANTS:
        found = re.findall(r"^\s*constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src, flags=re.M)
        assert len(found) == 1, "%s: %d constexpr lines in %s" % (name, len(found), SPARSE_LD)
        out[name] = int(found[0])
    return out


def column_lists(A, sub, short_below):
    """the two lists of plan_columns: the output positions whose column has at least `short_below` stored entries, then the
    rest, each in position order (A: full columns; sub: the column behind each position, None for all)"""
    L = np.diff(A.indptr)
    L = L if sub is None else L[np.asarray(sub)]
    return np.nonzero(L >= short_below)[0], np.nonzero(L < short_below)[0]


def as_full(A):
    A = sparse.csc_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    A.sort_indices()
    return A


def submatrix(A, sub):
    As = sparse.csc_matrix(A[sub][:, sub])
    As.sort_indices()
    return As


def csc_arrays(A):
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float64)


# ---- mixed_band: past the column stride of k_columns and the element stride of the vector kernels -------------------------------

def mixed_band(m2=280_000, n_long=10_000, half_long=40, seed=101):
    """Symmetric, unit diagonal; (i, j) is stored when |i - j| <= min(h_i, h_j), h = half_long for the first n_long columns
    and 1 for the rest.  Off-diagonals are uniform(-1, 1) x 0.004 where both ends are in the wide part and x 0.15 elsewhere:
    absolute off-diagonal row sums of at most 2 half_long 0.004 = 0.32 and 0.30."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for d in range(1, half_long + 1):
        i = np.arange(0, (m2 if d == 1 else n_long) - d)
        amp = np.where(i + d < n_long, 0.004, 0.15)
        rows.append(i)
        cols.append(i + d)
        vals.append(rng.uniform(-1, 1, i.size) * amp)
    up = sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m2, m2))
    return as_full(up + up.T + sparse.identity(m2))


def mixed_subset(A, short_below, n_short=70_000, seed=102):
    """every long column of A and n_short of its short ones, shuffled"""
    rng = np.random.default_rng(seed)
    long_, short = column_lists(A, None, short_below)
    return rng.permutation(np.concatenate([long_, rng.choice(short, n_short, replace=False)]))


def mixed_shift(m2, seed=103):
    """add_to_diag of the solve: uniform(0.1, 0.5)"""
    return np.random.default_rng(seed).uniform(0.1, 0.5, m2)


def mixed_rhs(m2, seed=108):
    return np.random.default_rng(seed).normal(size=m2)


def gershgorin(M):
    """[lo, hi] that holds the spectrum of the symmetric M: the union of the discs |z - M_jj| <= sum_{i != j} |M_ij|"""
    M = sparse.csc_matrix(M)
    c = M.diagonal()
    r = np.asarray(abs(M).sum(axis=0)).ravel() - np.abs(c)
    return float(np.min(c - r)), float(np.max(c + r))


def minres_iterations(kappa, t):
    """For a symmetric positive definite system MINRES satisfies ||r_k|| <= 2 ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^k ||b||
    (the Chebyshev bound of conjugate gradients holds for the residual-minimising method over the same Krylov space), so
    this many iterations suffice for a relative residual t."""
    s = math.sqrt(kappa)
    return int(math.ceil(math.log(2 / t) / math.log((s + 1) / (s - 1))))


# ---- aligned_columns: every cell of the pair loads of k_columns<., 64> --------------------------------------------------------

STEP = 128                                                    # entries per step of a wave: 64 lanes x one aligned pair
SHORT_SPECIALS = (0, 1, 62, 63, 64, 65)                       # both sides of the 63 / 64 boundary between the two kernels
LONG_SPECIALS = (127, 128, 129, 191, 192, 193, 255, 256, 257)


def aligned_columns(tail, m2=640, seed=104):
    """Full columns given directly, not symmetric: (p, i, x, m2, lengths).  The lengths are placed so that each of
    SHORT_SPECIALS and LONG_SPECIALS starts once at an even and once at an odd offset (a column of one entry in front
    flips the parity), the first column is long and starts at offset 0, and the last column is long; nnz is odd for
    tail="odd" and even for tail="even", so the last pair load ends in the allocation's slack or exactly at its edge.

    Rows.  Row 0 is stored nowhere; columns with an even index take their rows from the odd rows, columns with an odd index
    from the even rows >= 2.  The entries next to a column in memory belong to its neighbours, hence to the other class, so
    `poisoned_vector` can put 1e300 on every row that a wrongly kept half of a pair would gather without touching a term of
    the columns under test.  Only an empty neighbour (three columns, for the length 0) lets entries of the same class
    adjoin."""
    assert tail in ("odd", "even")
    rng = np.random.default_rng(seed)
    lengths = [129]
    for L in SHORT_SPECIALS + LONG_SPECIALS:
        for parity in (0, 1):
            if sum(lengths) % 2 != parity:
                lengths.append(1)
            lengths.append(L)
    lengths += list(rng.integers(1, 41, m2 - 1 - len(lengths)))
    last = 201
    if (sum(lengths) + last) % 2 != (1 if tail == "odd" else 0):
        last += 1
    lengths.append(last)
    lengths = np.array(lengths, dtype=np.int64)
    assert lengths.size == m2
    pools = (np.arange(1, m2, 2), np.arange(2, m2, 2))
    p = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    i = np.concatenate([np.sort(rng.choice(pools[c % 2], L, replace=False)) for c, L in enumerate(lengths)]).astype(np.int32)
    x = rng.uniform(-1, 1, i.size)
    x[x == 0] = 0.5
    return p, i, x, m2, lengths


def poisoned_vector(m2, klass, seed):
    """N(0, 1) on the rows that the columns of index parity `klass` store, 1e300 on every other row (row 0 and the rows of
    the other class): what a masked half of a pair load would gather"""
    v = np.random.default_rng(seed).normal(size=m2)
    clean = np.zeros(m2, dtype=bool)
    clean[(1 if klass == 0 else 2)::2] = True
    v[~clean] = POISON
    return v


def alignment_cells(p, lengths, short_below):
    """the (start parity, length parity, length mod 128) cells of the long columns"""
    return {(int(p[c] % 2), int(L % 2), int(L % STEP)) for c, L in enumerate(lengths) if L >= short_below}


# ---- wide_band: columns longer than one round of the coordinate kernels' column update ------------------------------------------

def wide_band(m2=3_000, half=1_100, seed=105):
    """Symmetric, unit diagonal, every entry within |i - j| <= half stored; off-diagonals uniform(-1, 1) x 0.3 / sqrt(2 half)"""
    rng = np.random.default_rng(seed)
    R = np.triu(rng.uniform(-1, 1, (m2, m2)) * (0.3 / math.sqrt(2 * half)), 1)
    R = R + R.T
    np.fill_diagonal(R, 1.0)
    ii, jj = np.nonzero(np.abs(np.subtract.outer(np.arange(m2), np.arange(m2))) <= half)
    return as_full(sparse.csc_matrix((R[ii, jj], (ii, jj)), shape=(m2, m2)))


def wide_subsets(m2, seed=107):
    """2 000 of the columns, sorted (the window path of the Gibbs sampler) and unsorted (its general path)"""
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(m2, 2000, replace=False)), rng.choice(m2, 2000, replace=False)


# the (lambda, delta) pairs and the chains that were tried on wide_band
WIDE_LAMBDA = np.array([0.08, 0.04, 0.01, 0.001])
WIDE_DELTA = np.array([0.001, 0.1, 1.0, 0.01])
WIDE_MAXITER = 30
WIDE_CHAINS = {"p": np.array([1.0, 0.05, 0.01]), "h2": np.full(3, 0.2), "sparse": np.array([False, False, True])}
WIDE_N = 1500.0
WIDE_BURN_IN, WIDE_NUM_ITER = 5, 10


def wide_beta_hat(m, seed=106):
    """beta_hat ~ N(0, 0.05^2)"""
    return np.random.default_rng(seed).normal(0, 0.05, m)


def df_of(beta_hat, n_eff):
    """summary statistics whose scale sqrt(n_eff beta_se^2 + beta^2) is 1 up to rounding, so that beta / scale is beta_hat
    (to an ulp; the tests derive the statement's input from the data frame, as the library does)"""
    beta_hat = np.asarray(beta_hat, dtype=np.float64)
    n_eff = np.broadcast_to(np.asarray(n_eff, dtype=np.float64), beta_hat.shape).copy()
    return {"beta": beta_hat.copy(), "beta_se": np.sqrt((1 - beta_hat ** 2) / n_eff), "n_eff": n_eff}


def take(df, sub):
    return df if sub is None else {k: np.asarray(v)[sub] for k, v in df.items()}


def gibbs_inputs(df):
    """R/LDpred2.R:110-114: (scale, beta_hat, n_eff)"""
    beta, se, n = (np.asarray(df[k], dtype=np.float64) for k in ("beta", "beta_se", "n_eff"))
    scale = np.sqrt(n * se ** 2 + beta ** 2)
    return scale, beta / scale, n


# ---- small systems: below, at and just above one block of 64 coordinates ------------------------------------------------------

SMALL_M = (1, 2, 63, 64, 65, 128, 129)
SMALL_M2 = 130


def banded_corr(m2, band, seed, n=60):
    rng = np.random.default_rng(seed)
    X = rng.binomial(2, rng.uniform(0.1, 0.5, m2), size=(n, m2)).astype(float)
    R = np.corrcoef(X, rowvar=False)
    R[np.isnan(R)] = 0
    jj, ii = np.meshgrid(np.arange(m2), np.arange(m2))
    R[np.abs(ii - jj) > band] = 0
    np.fill_diagonal(R, 1.0)
    return sparse.csc_matrix(R)


def small_whole(m):
    """banded_corr on m columns (np.corrcoef of one column is a scalar: the 1 x 1 matrix is written out)"""
    return as_full(sparse.csc_matrix(np.array([[1.0]])) if m == 1 else banded_corr(m, 6, seed=200 + m, n=500))


EMPTY_WITH_DIAGONAL, EMPTY = 40, 97


def small_with_empty_columns():
    """m2 = 130, band 6, symmetric; column (and row) 40 keeps its diagonal only, column (and row) 97 stores nothing"""
    E = sparse.lil_matrix(banded_corr(SMALL_M2, 6, seed=300, n=500))
    for j in (EMPTY_WITH_DIAGONAL, EMPTY):
        E[j, :] = 0
        E[:, j] = 0
    E[EMPTY_WITH_DIAGONAL, EMPTY_WITH_DIAGONAL] = 1.0
    A = sparse.csc_matrix(E)
    A.eliminate_zeros()
    return as_full(A)


def small_subsets(m, seed=301):
    """m of the 130 columns, ascending and shuffled; both hold the two empty columns whenever m >= 2"""
    rng = np.random.default_rng(seed + m)
    if m == 1:
        pick = np.array([EMPTY_WITH_DIAGONAL])
    else:
        rest = np.setdiff1d(np.arange(SMALL_M2), [EMPTY_WITH_DIAGONAL, EMPTY])
        pick = np.concatenate([[EMPTY_WITH_DIAGONAL, EMPTY], rng.choice(rest, m - 2, replace=False)])
    asc = np.sort(pick)
    shuffled = rng.permutation(pick)
    if m > 1 and np.all(np.diff(shuffled) > 0):
        shuffled = shuffled[::-1].copy()
    return asc, shuffled


def small_df(m, seed, sub=None):
    """summary statistics with unequal n_eff (a penalty factor other than 1) for a small system.  One position has a strong
    effect, so that every chain and grid point moves also when m is 1 or 2.  The position of the column that stores
    nothing has a beta below every lambda of the grid: its dot product stays 0 whatever its beta, so under a small delta a
    beta that moved would grow until the divergence stop turns the grid point into a NaN column."""
    rng = np.random.default_rng(seed)
    beta = rng.normal(0, 0.1, m)
    nothing = np.zeros(m, dtype=bool) if sub is None else np.asarray(sub) == EMPTY
    beta[np.nonzero(~nothing)[0][0]] = 0.4
    beta[nothing] = 0.001
    return {"beta": beta, "beta_se": rng.uniform(0.02, 0.04, m), "n_eff": np.round(rng.uniform(1200, 2000, m))}


def small_cases(m):
    """(name, full matrix, ind_corr, summary statistics) of a small system of m coordinates: the whole m x m matrix, and m
    of the 130 columns of the matrix with empty columns, ascending and shuffled"""
    E = small_with_empty_columns()
    asc, shuffled = small_subsets(m)
    return [("whole", small_whole(m), None, small_df(m, 400 + m)), ("ascending", E, asc, small_df(m, 500 + m, asc)),
            ("shuffled", E, shuffled, small_df(m, 600 + m, shuffled))]


SMALL_LASSO = {"nlambda": 4, "delta": (0.01, 1.0), "maxiter": 50}
SMALL_CHAINS = {"p": np.array([1.0, 0.1, 0.01]), "h2": np.full(3, 0.3), "sparse": np.array([False, False, True])}
SMALL_BURN_IN, SMALL_NUM_ITER = 5, 10


def repeated_subset(seed=302):
    """200 positions over the 130 columns: a permutation of all columns, then 70 repeats.  Positions 3 and 9 hold one
    column and 20, 21 another (repeats inside the first block of 64 positions); positions 130 .. 199 repeat columns of
    positions 0 .. 129 (across blocks), and 190, 191 repeat each other inside the fourth block."""
    rng = np.random.default_rng(seed)
    ind = np.concatenate([rng.permutation(SMALL_M2), rng.integers(0, SMALL_M2, 70)])
    ind[9] = ind[3]
    ind[21] = ind[20]
    ind[191] = ind[190]
    return ind.astype(np.int64)


def lassosum2_statement(ref, A, df, sub=None, delta=(0.001, 0.01, 0.1, 1), nlambda=30, lambda_min_ratio=0.01, **kw):
    """the CPU statement `ref.grid` on the full columns of A with snp_lassosum2's inputs (R/lassosum2.R:49-57) from df, the
    summary statistics of the listed positions; scaled back as R/lassosum2.R:80 does: (beta, num_iter, sparsity, moves)"""
    from bigsnpr_amd.lassosum2 import _col_means_zero, lassosum2_inputs
    fp, fi, fx = csc_arrays(A)
    scale, bh, pf, lam, dl = lassosum2_inputs(np.asarray(df["beta"], dtype=np.float64), np.asarray(df["beta_se"], dtype=np.float64),
                                              np.asarray(df["n_eff"], dtype=np.float64), delta, nlambda, lambda_min_ratio)
    beta, iters, moves, _ = ref.grid(fp, fi, fx, A.shape[0], bh, pf, lam, dl, ind_sub=sub, nthreads=16, **kw)
    return beta * scale[:, None], iters, _col_means_zero(beta), moves


def gibbs_statement(ref, A, df, gp, seed, sub=None, burn_in=50, num_iter=100):
    """the CPU statement `ref.grid` with snp_ldpred2_grid's inputs from df, scaled back as R/LDpred2.R:139 does: (beta, moves)"""
    fp, fi, fx = csc_arrays(A)
    scale, bh, n = gibbs_inputs(df)
    beta, moves, _ = ref.grid(fp, fi, fx, A.shape[0], bh, n, gp["h2"], gp["p"], gp["sparse"], ind_sub=sub, stream=gp.get("stream"),
                              burn_in=burn_in, num_iter=num_iter, seed=seed, nthreads=16)
    return beta * scale[:, None], moves


# ---- LDpred2-auto on the inputs above, and the inputs that only k_ldpred2_auto needs ------------------------------------------

AUTO_SEED = 2024
AUTO_WIDE = {"vec_p_init": (1.0, 0.05, 0.01), "h2_init": 0.2, "burn_in": WIDE_BURN_IN, "num_iter": WIDE_NUM_ITER, "report_step": 3}
AUTO_SMALL = {"vec_p_init": (1.0, 0.1, 0.01), "h2_init": 0.3, "burn_in": SMALL_BURN_IN, "num_iter": SMALL_NUM_ITER,
              "report_step": 4}


def full_of(A):
    """(p, i, x, m2) of the full columns, as the statements take them"""
    return csc_arrays(A) + (A.shape[0],)


def wide_auto_cases(A):
    """(name, ind_corr, summary statistics, ascending) of the three selections of wide_band under auto"""
    m2 = A.shape[0]
    df = df_of(wide_beta_hat(m2), WIDE_N)
    srt, uns = wide_subsets(m2)
    return [("whole", None, df, True), ("ascending", srt, take(df, srt), True), ("unsorted", uns, take(df, uns), False)]


STRADDLE_M = 320
STRADDLE = {"vec_p_init": (0.7,), "h2_init": 0.2, "p_bounds": (0.7, 0.7), "burn_in": 5, "num_iter": 25, "report_step": 1}


def straddle_case():
    """320 coordinates of which p = 0.7 (held there by p_bounds) keeps about 260 causal: the size of the causal set after a
    sweep falls on both sides of the stride of the epilogue's loops (kGibbsThreads) and on it"""
    return as_full(banded_corr(STRADDLE_M, 6, seed=900, n=500)), small_df(STRADDLE_M, 901)


WINDOW_LIMIT_M2 = 20_000
WINDOW_LIMIT = {"vec_p_init": (1.0, 0.05, 0.01), "h2_init": 0.2, "burn_in": 5, "num_iter": 10, "report_step": 4, "use_MLE": True}


def window_limit_cases(W, m2=WINDOW_LIMIT_M2):
    """The summary statistics and the two matrices of test_window_limit in tests/test_gpu_ldpred2_grid.py, from the same
    generator in the same order: a few entries per column, one of them `half` rows from the diagonal, so an envelope of
    2 half + 64 rows.  W: the rows of the largest LDS window.  Yields (half, fits, A, df)."""
    rng = np.random.default_rng(17)
    df = {"beta": rng.normal(0, 0.05, m2), "beta_se": np.full(m2, 0.03), "n_eff": np.full(m2, 1500.0)}
    for half, fits in ((W // 2 - 40, True), (W // 2, False)):
        d = np.arange(m2 - half)
        far = sparse.coo_matrix((rng.uniform(-0.05, 0.05, d.size), (d, d + half)), shape=(m2, m2))
        near = sparse.diags([rng.uniform(-0.3, 0.3, m2 - 1)], [1])
        up = sparse.csc_matrix(far + near)
        yield half, fits, as_full(sparse.csc_matrix(up + up.T + sparse.identity(m2))), df


def diverging_case(m2=200):
    """the matrix and summary statistics of test_divergence_gives_the_statements_nan_pattern (tests/test_gpu_ldpred2_auto.py):
    0.9 on the first two off-diagonals, not positive definite"""
    A = sparse.csc_matrix(sparse.diags([np.full(m2 - 2, 0.9), np.full(m2 - 1, 0.9), np.ones(m2), np.full(m2 - 1, 0.9),
                                        np.full(m2 - 2, 0.9)], [-2, -1, 0, 1, 2]))
    rng = np.random.default_rng(17)
    return as_full(A), {"beta": rng.normal(0, 0.05, m2), "beta_se": np.full(m2, 0.03), "n_eff": np.full(m2, 1500.0)}


# ---- the batch loops of the three drivers -------------------------------------------------------------------------------------

BATCH_CAPS = (1, 2, 4)               # of 5 chains: 5 batches of 1; 2, 2, 1; 4, 1.  Of the 8 grid points of SMALL_LASSO: 8, 4, 2 batches
BATCH_CAPS_LASSO = (1, 2, 3, 4)      # 3: batches of 3, 3, 2, a last batch shorter than the others for the grid of 8 as well
BATCH_M = 65
# five chains: unequal p in an order that is not the sorted one (the drivers visit large p first), stream ids that are not 0 .. 4
BATCH_CHAINS = {"p": np.array([0.03, 1.0, 0.005, 0.3, 0.1]), "h2": np.array([0.3, 0.2, 0.3, 0.25, 0.3]),
                "sparse": np.array([False, False, True, False, True]), "stream": np.array([7, 3, 11, 5, 20], dtype=np.uint64)}
BATCH_AUTO = {"vec_p_init": (0.03, 1.0, 0.005, 0.3, 0.1), "stream": np.array([7, 3, 11, 5, 20], dtype=np.uint64), "h2_init": 0.3,
              "burn_in": SMALL_BURN_IN, "num_iter": SMALL_NUM_ITER, "report_step": 4}


def batch_cases():
    """(name, full matrix, ind_corr, summary statistics): the 130 columns of small_with_empty_columns, and BATCH_M of them
    ascending and shuffled (both hold the two empty columns)"""
    E = small_with_empty_columns()
    asc, shuffled = small_subsets(BATCH_M)
    return [("whole", E, None, small_df(SMALL_M2, 800, np.arange(SMALL_M2))), ("ascending", E, asc, small_df(BATCH_M, 801, asc)),
            ("shuffled", E, shuffled, small_df(BATCH_M, 802, shuffled))]
