"""Inputs and plain NumPy restatements shared by tests/test_knn_cpu.py and tests/test_gpu_knn.py (knn_parallel, prob_dist,
LOF: bigsnpr_amd/csrc/knn_step.hpp is the statement, tests/native/knn_ref.py its CPU twin)."""
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
