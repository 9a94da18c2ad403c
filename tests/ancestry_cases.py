"""Shared by tests/test_ancestry_cpu.py and tests/test_gpu_ancestry.py: the quadratic programs of the case list C1 with
the checks against the definition (feasibility, KKT), and the planted-mixture tables of C3 on the golden .bed files."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CAP = 60   # qp::kMaxK


# ---- the program against its definition ---------------------------------------------------------------------------------
def objective(D, d, w):
    return 0.5 * w @ D @ w - d @ w


def tol_kkt(D, d):
    """1e-10 (max|D| + max|d|): backward stability of the factor updates gives about K 2^-53 |D| |w| with |w|_1 <= 1"""
    return 1e-10 * (np.abs(D).max() + np.abs(d).max())


def kkt_residuals(D, d, w, sum_to_one):
    """(stationarity, most negative multiplier of an inequality as a positive number, complementary slackness), the
    multipliers recovered by least squares on the active set: D w - d = sum_k mu_k e_k - lambda 1"""
    K = w.size
    g = D @ w - d
    bounds = [k for k in range(K) if w[k] <= 1e-12]
    sum_active = sum_to_one or abs(w.sum() - 1.0) <= 1e-12
    cols = [np.eye(K)[:, k] for k in bounds] + ([-np.ones(K)] if sum_active else [])
    if not cols:
        return np.abs(g).max(), 0.0, 0.0
    N = np.array(cols).T
    u = np.linalg.lstsq(N, g, rcond=None)[0]
    ineq = list(u[:len(bounds)]) + ([u[-1]] if sum_active and not sum_to_one else [])
    slack = [abs(w[k] * u[i]) for i, k in enumerate(bounds)] + ([abs((1.0 - w.sum()) * u[-1])] if sum_active else [])
    return np.abs(g - N @ u).max(), max([0.0] + [-v for v in ineq]), max(slack)


def check_solution(D, d, w, sum_to_one, what=""):
    """the C1 checks on one solution; returns the worst KKT residual over tol_kkt"""
    assert np.isfinite(w).all(), (what, w)
    assert w.min() >= -1e-12, (what, w.min())
    if sum_to_one:
        assert abs(w.sum() - 1.0) <= 1e-12, (what, w.sum() - 1.0)
    else:
        assert w.sum() <= 1.0 + 1e-12, (what, w.sum() - 1.0)
    tol = tol_kkt(D, d)
    res = kkt_residuals(D, d, w, sum_to_one)
    assert max(res) <= tol, (what, res, tol)
    return max(res) / tol


def slsqp(D, d, sum_to_one):
    """the minimiser by scipy's SLSQP (the looser of the two: it recovers a planted mixture to about 5e-6)"""
    from scipy.optimize import minimize
    K = d.size
    cons = [dict(type="eq" if sum_to_one else "ineq", fun=lambda w: 1.0 - w.sum(), jac=lambda w: -np.ones(K))]
    r = minimize(lambda w: objective(D, d, w), np.full(K, 1.0 / K), jac=lambda w: D @ w - d, method="SLSQP", bounds=[(0.0, None)] * K,
                 constraints=cons, options=dict(ftol=1e-15, maxiter=2000))
    return r.x


def _spd(rng, K, extra=3):
    A = rng.normal(size=(K + extra, K))
    return A.T @ A / (K + extra)


def qp_cases(nearPD):
    """[(name, D, d, sum_to_one, w_known or None)]: every finite case of the list C1"""
    rng = np.random.default_rng(20221)
    out = []
    for K in (1, 2, 3):
        D = _spd(rng, K)
        for s1 in (True, False):
            out.append(("K%d_%s" % (K, s1), D, rng.normal(size=K), s1, None))
    K = 7
    D = _spd(rng, K)
    wi = rng.dirichlet(np.ones(K) * 5.0)
    out.append(("interior", D, D @ wi, True, wi))                                   # the unconstrained minimum sums to 1
    e = np.zeros(K)
    e[2] = 1.0
    mu = np.ones(K)
    mu[2] = 0.0
    out.append(("vertex", D, D @ e - mu + 0.5, True, e))                            # K - 1 bounds active
    out.append(("below_one", D, D @ (0.5 * wi), False, 0.5 * wi))                   # sum w = 1/2
    out.append(("all_negative", D, -np.abs(rng.normal(size=K)) - 0.1, False, np.zeros(K)))
    X = rng.normal(size=(9, K))
    X[:, 1] = X[:, 0]                                                               # two identical reference columns
    Dn, ok = nearPD(X.T @ X)
    assert ok
    wt = np.zeros(K)
    wt[[3, 5]] = 0.7, 0.3
    for s1 in (True, False):
        out.append(("twins_%s" % s1, Dn, X.T @ (X @ wt), s1, None))
    D = _spd(rng, CAP, 10)
    wt = np.zeros(CAP)
    wt[[0, 17, 59]] = 0.5, 0.3, 0.2
    for s1 in (True, False):
        out.append(("cap_%s" % s1, D, D @ wt + 0.05 * rng.normal(size=CAP), s1, None))
    return out


def problem_batch(K, B, seed, nearPD=None):
    """(D, d: K x B) for the shape tests: mixtures of planted sparse weights, noise and unconstrained directions.  With
    nearPD: D = nearPD(X'X) of an L = K - 2 < K projection (condition about 1e8), d in the range of X'"""
    rng = np.random.default_rng(seed)
    if nearPD is not None and K > 2:
        X = rng.normal(size=(K - 2, K))
        D, ok = nearPD(X.T @ X)
        assert ok
        W = rng.dirichlet(np.ones(K) * 0.3, size=B).T
        return D, X.T @ (X @ W + 0.1 * rng.normal(size=(K - 2, B)))
    D = _spd(rng, K)
    W = rng.dirichlet(np.ones(K) * 0.3, size=B).T
    return D, D @ W + 0.3 * rng.normal(size=(K, B)) * (np.arange(B) % 3)


# ---- the golden files ----------------------------------------------------------------------------------------------------
def read_bed(prefix):
    """(G: n x m allele counts as doubles, NaN = missing; the family labels)"""
    with open(prefix + ".fam") as f:
        fam = [line.split()[0] for line in f if line.strip()]
    with open(prefix + ".bim") as f:
        m = sum(1 for line in f if line.strip())
    n = len(fam)
    raw = np.fromfile(prefix + ".bed", dtype=np.uint8)
    assert raw[0] == 0x6C and raw[1] == 0x1B and raw[2] == 1
    nb = (n + 3) // 4
    by = raw[3:].reshape(m, nb)
    codes = np.stack([(by >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(m, nb * 4)[:, :n]
    G = np.array([2.0, np.nan, 1.0, 0.0])[codes].T
    return np.asfortranarray(G), fam


def tables(G, groups, L):
    """X0: the allele frequency of every group (list of row-index arrays), m x K; P: the first L right singular vectors of
    the binomially scaled matrix, divided by the scale, m x L; correction: ones"""
    X0 = np.asfortranarray(np.stack([np.nanmean(G[g], axis=0) / 2.0 for g in groups], axis=1))
    p = np.nanmean(G, axis=0) / 2.0
    scale = np.sqrt(2.0 * p * (1.0 - p))
    ok = scale > 0
    Z = np.where(np.isnan(G), 2.0 * p, G) - 2.0 * p
    Z[:, ok] /= scale[ok]
    Z[:, ~ok] = 0.0
    V = np.linalg.svd(Z, full_matrices=False)[2][:L].T
    P = np.zeros_like(V)
    P[ok] = V[ok] / scale[ok, None]
    return X0, np.asfortranarray(P), np.ones(L)


def example_tables(L):
    """C3: example.bed (517 x 4542, no missing value), the 19 family labels POP1 .. POP19 as the reference groups"""
    G, fam = read_bed(os.path.join(GOLDEN, "example"))
    labels = ["POP%d" % k for k in range(1, 20)]
    fam = np.array(fam)
    groups = [np.nonzero(fam == lab)[0] for lab in labels]
    X0, P, corr = tables(G, groups, L)
    wt = np.zeros(19)
    wt[[0, 7, 15]] = 0.6, 0.3, 0.1
    own = np.array([labels.index(f) for f in fam])
    return dict(G=G, X0=X0, P=P, corr=corr, wt=wt, freq=X0 @ wt, own=own)


def missing_tables(K=5, L=3):
    """G6: example-missing.bed (200 x 500), samples i = k mod K as reference group k"""
    G, _ = read_bed(os.path.join(GOLDEN, "example-missing"))
    groups = [np.arange(k, G.shape[0], K) for k in range(K)]
    X0, P, corr = tables(G, groups, L)
    return dict(G=G, X0=X0, P=P, corr=corr)
