"""knn_parallel / prob_dist / LOF — outlier samples in PCA scores, host mirror of the three bigutilsr functions that the
reference's PCA workflow calls between its two bed_autoSVD runs (vignettes/bedpca.Rmd: `bigutilsr::prob_dist(obj.svd$u)`,
`S <- dist.self / sqrt(dist.nn)`), over bsn_knn / bsn_prob_dist / bsn_lof (bigsnpr_amd/csrc/knn.hip).

The search is exact and exhaustive — every pair of a query and a data point, in fp64, on the device: at 400 000 x 20
scores a tree search degenerates to brute force anyway.

bigutilsr's own nearest-neighbour search and its handling of ties are NOT emulated: the package is external to the
reference tree, its source is not at hand and no R exists here to pin it against.  The rule used instead is stated in
full in csrc/knn_step.hpp and DESIGN.md 3.5r, and pinned against a CPU statement compiled from that header:

    squared distance   acc = 0; for d = 0 .. p - 1: t = q[d] - x[d], acc = fma(t, t, acc)
    order              candidates ascending by (squared distance, 0-based index of the data point)
    self mode          `query=None`: the candidate with the query's own index is left out — by index, not by distance;
                       other rows equal to the query stay in, at distance 0.  (bigutilsr asks for k + 1 neighbours and
                       drops the first column, which on duplicated rows may drop a twin and keep the point itself: a
                       deliberate difference.)
    prob_dist          m2[i] = mean of i's kNN squared distances, dist_self = sqrt(m2), dist_nn[i] = mean of m2 over
                       i's neighbours; S = dist_self / sqrt(dist_nn) is the vignette's statistic
    LOF                Breunig, Kriegel, Ng & Sander 2000, for every k of `seq_k`, combined over k by `combine`

PARITY STATUS of this module: **unpinned** against bigutilsr, as for `king_norel` and `indep_pairwise`."""
import numpy as np

from . import _lib
from ._lib import check, f64p, i32p, ptr
from .bed import ERROR_DIM

MAX_P = MAX_K = 64


def _matrix(a, name):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("'%s' should be a matrix with at least one row and one column." % name)
    return a


def _check_k(k, n_cand, name="k"):
    if int(k) != k:
        raise ValueError("'%s' should be an integer." % name)
    k = int(k)
    if k < 1 or k > MAX_K:
        raise ValueError("'%s' should be in range [1, %d] (got %d)." % (name, MAX_K, k))
    if k > n_cand:
        raise ValueError("'%s' should be at most %d here (got %d)." % (name, n_cand, k))
    return k


def _check_p(p):
    if p > MAX_P:
        raise ValueError("at most %d columns (got %d)." % (MAX_P, p))


def knn_parallel(data, query=None, k=None):
    """The `k` nearest data points of every query: dict(nn_idx, nn_dists), nq x k each, neighbours in ascending order of
    (distance, index).  nn_idx is int32 and 0-based.  `query=None` is self mode: the data is its own query and a point is
    not its own neighbour (left out by index; its duplicates stay in, at distance 0)."""
    if k is None:
        raise TypeError("knn_parallel: 'k' is missing")
    data = _matrix(data, "data")
    n, p = data.shape
    _check_p(p)
    if query is not None:
        query = _matrix(query, "query")
        if query.shape[1] != p:
            raise ValueError(ERROR_DIM)
    nq = n if query is None else query.shape[0]
    k = _check_k(k, n - 1 if query is None else n)
    L = _lib.load()
    idx = np.empty((nq, k), dtype=np.int32, order="F")
    dist = np.empty((nq, k), order="F")
    d_data = _lib.DeviceArray.from_numpy(data)
    d_query = None if query is None else _lib.DeviceArray.from_numpy(query)
    try:
        check(L.bsn_knn(d_data.ptr, n, n, None if d_query is None else d_query.ptr, nq, nq, p, k, ptr(idx, i32p), ptr(dist, f64p)))
    finally:
        d_data.free()
        if d_query is not None:
            d_query.free()
    return dict(nn_idx=idx, nn_dists=dist)


def rob_maha(U):
    """U E diag(1 / sqrt(lambda)), (E, lambda) the eigen-decomposition of the robust covariance of U (the orthogonalised
    Gnanadesikan-Kettenring estimate, autosvd.covrob_ogk_device): Euclidean distances between its rows are robust
    Mahalanobis distances between the rows of U.  What `robMaha=True` searches in."""
    from .autosvd import covrob_ogk_device
    U = _matrix(U, "U")
    _check_p(U.shape[1])
    lam, E = np.linalg.eigh(covrob_ogk_device(U)["cov"])
    return (U @ E) / np.sqrt(lam)


def prob_dist(U, kNN=5, robMaha=False):
    """bigutilsr::prob_dist: dict(dist_self, dist_nn, S).  dist_self[i] is the root-mean-square distance of row i to its
    `kNN` nearest rows, dist_nn[i] the mean over those neighbours of their own mean squared distance, and
    S = dist_self / sqrt(dist_nn) the vignette's statistic (LoOP's PLOF + 1): a threshold on S names the outlier samples."""
    U = _matrix(U, "U")
    n, p = U.shape
    _check_p(p)
    kNN = _check_k(kNN, n - 1, "kNN")
    if robMaha:
        U = rob_maha(U)
    L = _lib.load()
    ds, dn = np.empty(n), np.empty(n)
    d_U = _lib.DeviceArray.from_numpy(U)
    try:
        check(L.bsn_prob_dist(d_U.ptr, n, n, p, kNN, ptr(ds, f64p), ptr(dn, f64p)))
    finally:
        d_U.free()
    with np.errstate(divide="ignore", invalid="ignore"):
        S = ds / np.sqrt(dn)
    return dict(dist_self=ds, dist_nn=dn, S=S)


def lof_matrix(U, seq_k=(4, 10, 30), robMaha=False):
    """the n x len(seq_k) matrix of local outlier factors, one column per number of neighbours, as the library returns it"""
    U = _matrix(U, "U")
    n, p = U.shape
    _check_p(p)
    seq = np.atleast_1d(np.asarray(seq_k))
    if seq.ndim != 1 or seq.size < 1:
        raise ValueError("'seq_k' should be a non-empty vector.")
    seq = np.ascontiguousarray([_check_k(kk, n - 1, "seq_k") for kk in seq], dtype=np.int32)
    if robMaha:
        U = rob_maha(U)
    L = _lib.load()
    out = np.empty((n, seq.size), order="F")
    d_U = _lib.DeviceArray.from_numpy(U)
    try:
        check(L.bsn_lof(d_U.ptr, n, n, p, ptr(seq, i32p), seq.size, ptr(out, f64p)))
    finally:
        d_U.free()
    return out


def LOF(U, seq_k=(4, 10, 30), combine=max, robMaha=False, log=True):
    """bigutilsr::LOF: the local outlier factor of every row, computed for every number of neighbours of `seq_k` and
    combined over them by `combine` (any callable over the values of one row; the builtin `max`, the default, is taken
    column-wise in one step), in log scale unless `log=False`.  Duplicated rows give inf and NaN, as IEEE has them."""
    M = lof_matrix(U, seq_k, robMaha)
    if combine is max or combine is np.max:
        v = M.max(axis=1)
    elif combine is min or combine is np.min:
        v = M.min(axis=1)
    else:
        v = np.array([combine(row) for row in M], dtype=np.float64)
    if log:
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.log(v)
    return v


def knn_last_stats():
    """device milliseconds of the last knn_parallel / prob_dist / LOF call of this process — pack, scan, merge, rest — and
    the slab count and queries per workgroup it ran with"""
    out = np.zeros(6)
    check(_lib.load().bsn_knn_last_stats(ptr(out, f64p)))
    return dict(pack_ms=out[0], scan_ms=out[1], merge_ms=out[2], rest_ms=out[3], slabs=int(out[4]), query_block=int(out[5]))
