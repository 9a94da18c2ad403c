"""Inputs, the sweep over the scan kernels and plain NumPy restatements shared by tests/test_knn_cpu.py,
tests/test_gpu_knn.py and tests/test_gpu_knn_shapes.py (knn_parallel, prob_dist, LOF: bigsnpr_amd/csrc/knn_step.hpp is the
statement, tests/native/knn_ref.py its CPU twin)."""
import numpy as np

PLANTED = 5     # isolated far points at the end of planted_outliers()


def lattice(n, p, side, seed):
    """n points with integer coordinates 0 .. side - 1: every squared distance is exact in any order of summation, and
    there are many exact ties and duplicated rows"""
    return np.random.default_rng(seed).integers(0, side, size=(n, p)).astype(np.float64)


def grid_ties(seed=11):
    """600 points on the 5 x 5 x 5 integer grid: each grid point about 4.8 times, so ties run through and across the
    k-th place for k = 31"""
    g = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    pts = np.concatenate([np.tile(g, (4, 1)), g[rng.integers(0, 125, size=100)]])
    return pts[rng.permutation(600)]


def scores(n, p, seed):
    """standard-normal scores scaled like the u of a partial SVD (unit columns)"""
    return np.random.default_rng(seed).normal(size=(n, p)) / np.sqrt(n)


def planted_outliers(seed=5):
    """three Gaussian clusters of 300 points in p = 10 and, last, PLANTED isolated points far from all of them and from
    each other"""
    rng = np.random.default_rng(seed)
    p = 10
    centres = rng.normal(size=(3, p)) * 6.0
    X = np.concatenate([c + rng.normal(size=(300, p)) for c in centres])
    far = np.zeros((PLANTED, p))
    for t in range(PLANTED):
        far[t, t] = 60.0 * (1 if t % 2 == 0 else -1)
        far[t, PLANTED + t] = 45.0
    return np.concatenate([X, far])


# ---- the sweep over the scan kernels ---------------------------------------------------------------------------------
# knn.hip compiles one k_knn_scan<P, QL> per padded coordinate count P = 4, 8, .., 64 and queries per lane QL (2 only for
# P <= 32), each with its own register budget and unroll factor U = (P * QL <= 32 ? 4 : 2).  The sweep reaches every one:
#   p = P - 3 and P   three zero-padded coordinates and none
#   k = 5 and 17      blocks of 256 queries (QL = 2 where P <= 32) and of 128 (QL = 1)
#   n = 513           three blocks of 256, the last of ONE query (lane 0 holds a valid and an invalid query under QL = 2),
#                     or five blocks of 128
#   S = 1 and 3       one run of 16 tiles of 32 + 1 point, or slabs of 171 = 5 tiles + 11: both tails are odd, so the
#                     `jj + u < cnt` guard is live for U = 4 and for U = 2
SWEEP_P = tuple(range(4, 65, 4))
SWEEP_K = (5, 17)
SWEEP_N = 513
SWEEP_S = (1, 3)
SWEEP_QUERY_P = (8, 32, 36, 64)      # the P that the device tests also run in query mode


def instantiation(p, k):
    """(P, qb, QL) of a call with p coordinates and k neighbours: knn_plan.hpp's padded_p and query_block, knn.hip's
    queries_per_lane.  tests/test_knn_cpu.py holds this restatement to the two sources."""
    P = (p + 3) // 4 * 4
    qb = 256 if k <= 16 else 128 if k <= 32 else 64
    return P, qb, 2 if P <= 32 and qb == 256 else 1


def sweep(P=None):
    """the (p, k, S) of the sweep, all of them or those of one P"""
    return [(p, k, S) for PP in (SWEEP_P if P is None else (P,)) for p in (PP - 3, PP) for k in SWEEP_K for S in SWEEP_S]


def queries_with_copies(X, nq, seed, make):
    """nq queries from make(nq, p, seed), the first, the middle and the last of them copied from the data: the row
    numbers copied, and the queries"""
    n = X.shape[0]
    rows = [1, n // 2, n - 1]
    Q = make(nq, X.shape[1], seed)
    Q[[0, nq // 2, nq - 1]] = X[rows]
    return rows, Q


HUGE = 1e200      # finite, and the square of any difference with an ordinary coordinate overflows to +inf


def with_huge(n, p, seed):
    """a lattice of n points (p >= 3) in which every fifth row or so has +-HUGE in coordinate 0, 2 or both: rows of the
    same pattern are at exact finite squared distances from each other, rows of different patterns at +inf (an overflow
    of finite coordinates); a pattern has n / 25 members or so, fewer than a list has places.  The data, and a query
    set whose last two rows hold patterns no data row has (every candidate at +inf: the index alone orders them)."""
    rng = np.random.default_rng(seed)
    X = lattice(n, p, 4, seed)
    patterns = [(HUGE, None), (-HUGE, None), (None, HUGE), (HUGE, HUGE), (-HUGE, HUGE)]
    rows = rng.permutation(n)[: n // 5]
    for t, r in enumerate(rows):
        a, b = patterns[t % 5]
        if a is not None:
            X[r, 0] = a
        if b is not None:
            X[r, 2] = b
    Q = np.concatenate([lattice(9, p, 4, seed + 1), X[rows[:6]], lattice(2, p, 4, seed + 2)])
    Q[-2, 2] = -HUGE                 # no data row has this pattern
    Q[-1, 1] = HUGE
    return X, Q


# ---- NumPy restatements ----------------------------------------------------------------------------------------------
def np_d2(data, query=None):
    """all squared distances, nq x n (NumPy has no fma: exact on a lattice, within (p + 2) half-ulps otherwise)"""
    q = data if query is None else query
    t = q[:, None, :] - data[None, :, :]
    return (t * t).sum(axis=2)


def np_knn(data, query=None, k=1, d2=None):
    """the k smallest by (squared distance, index), the own index removed in self mode: nn_idx, nn_d2 (nq x k)"""
    d2 = np_d2(data, query) if d2 is None else d2
    nq, n = d2.shape
    idx = np.empty((nq, k), dtype=np.int32)
    for i in range(nq):
        order = np.lexsort((np.arange(n), d2[i]))
        if query is None:
            order = order[order != i]
        idx[i] = order[:k]
    return idx, np.take_along_axis(d2, idx.astype(np.int64), axis=1)


def np_prob_dist(idx, d2):
    k = idx.shape[1]
    m2 = d2[:, 0].copy()
    for t in range(1, k):
        m2 = m2 + d2[:, t]
    m2 = m2 / k
    s = m2[idx[:, 0]].copy()
    for t in range(1, k):
        s = s + m2[idx[:, t]]
    return np.sqrt(m2), s / k


def np_lof(idx, dist, seq_k):
    out = np.empty((idx.shape[0], len(seq_k)))
    for c, kk in enumerate(seq_k):
        kdist = dist[:, kk - 1]
        reach = np.maximum(kdist[idx[:, :kk]], dist[:, :kk])
        with np.errstate(divide="ignore", invalid="ignore"):
            lrd = 1.0 / (reach.sum(axis=1) / kk)
            out[:, c] = (lrd[idx[:, :kk]].sum(axis=1) / kk) / lrd
    return out
