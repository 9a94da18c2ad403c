"""Shared by tests/test_ancestry_cpu.py, tests/test_gpu_ancestry.py and tests/test_gpu_ancestry_shapes.py: the quadratic
programs of the case list C1 with the checks against the definition (feasibility, KKT), the planted-mixture tables of C3 on
the golden .bed files, and the synthetic tables of the shape sweep (a correction that is not all ones, every group width)."""
import functools
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


def same_minimiser(D, d, got, want, s1, what):
    """one device solution against the statement's on the same D and d: objectives, and the C1 checks on the device's w;
    returns the worst KKT residual over tol_kkt"""
    f, fr = objective(D, d, got), objective(D, d, want)
    assert abs(f - fr) <= 1e-12 * (1.0 + abs(fr)), (what, f, fr)
    return check_solution(D, d, got, s1, what)


def group_width(K):
    """lanes of a wave that k_anc_qp gives one problem"""
    return 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64


def per_workgroup(K):
    return 64 // group_width(K)


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
    return X0, projection(G, L), np.ones(L)


def projection(G, L):
    """P of tables()"""
    p = np.nanmean(G, axis=0) / 2.0
    scale = np.sqrt(2.0 * p * (1.0 - p))
    ok = scale > 0
    Z = np.where(np.isnan(G), 2.0 * p, G) - 2.0 * p
    Z[:, ok] /= scale[ok]
    Z[:, ~ok] = 0.0
    V = np.linalg.svd(Z, full_matrices=False)[2][:L].T
    P = np.zeros_like(V)
    P[ok] = V[ok] / scale[ok, None]
    return np.asfortranarray(P)


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


# ---- the shape sweep: synthetic tables with a real correction ----------------------------------------------------------------
def synthetic_tables(n, m, K, L, seed, na=0.0):
    """dict(G, X0, P, corr).  X0 (m x K): a base frequency U(0.1, 0.9) per variant plus 0.12 N(0, 1) per population, clipped
    to [0.02, 0.98] (no NaN, whatever `na`); G (n x m doubles, NaN = missing): sample i drawn binomial(2, .) from population
    i mod K, a share `na` of the cells missing; P as tables() forms it; corr = 1 + 0.013 j^1.5: distinct and increasing, as
    the reference's corrections are (up to about 7.5 at L = 64)"""
    assert n >= L + 6, "the centred n x m matrix must have L directions"
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.1, 0.9, size=m)
    X0 = np.clip(base[:, None] + 0.12 * rng.normal(size=(m, K)), 0.02, 0.98)
    G = rng.binomial(2, X0[:, np.arange(n) % K].T).astype(np.float64)
    if na > 0:
        G[rng.uniform(size=(n, m)) < na] = np.nan
    G = np.asfortranarray(G)
    return dict(G=G, X0=np.asfortranarray(X0), P=projection(G, L), corr=1.0 + 0.013 * np.arange(L) ** 1.5)


# two K per group width of k_anc_qp, on both sides of each boundary, then two tables with L < K (cond(Dmat) about 1e8)
SHAPE_SWEEP = [(1, 1), (8, 8), (9, 12), (16, 20), (17, 20), (32, 40), (33, 40), (60, 64), (19, 5), (60, 10)]
RANK_DEFICIENT = [(19, 5), (60, 10)]
SWEEP_SEED = {kl: 7000 + 100 * kl[0] + kl[1] for kl in SHAPE_SWEEP}   # chosen in tests/test_ancestry_cpu.py (the input claims)


def sweep_counts(K):
    """problem counts around a workgroup of k_anc_qp"""
    pw = per_workgroup(K)
    return sorted({b for b in (1, pw - 1, pw, pw + 1, 4 * pw + 3) if b >= 1})


def sweep_dims(K, L):
    """(n, m) of the image of one sweep entry: m is no multiple of 4, 64 or 512; n holds the largest problem count and the
    L directions"""
    return max(4 * per_workgroup(K) + 3, L + 6), 301 if K <= 19 else 523


@functools.lru_cache(maxsize=None)
def sweep_tables(K, L, na=0.0):
    """the tables of one sweep entry; made once, shared by the tests and left unchanged"""
    n, m = sweep_dims(K, L)
    t = synthetic_tables(n, m, K, L, SWEEP_SEED[(K, L)], na)
    for a in t.values():
        a.setflags(write=False)
    return t


def fill_missing(G, X0):
    """a missing cell counts as 2 c_j, c_j = mean_k X0[j, k]: what bed_ancestry makes of it"""
    return np.where(np.isnan(G), 2.0 * X0.mean(axis=1)[None, :], G)


def frequency_columns(t, B, seed):
    """M x B frequency columns for the summary path, column b a function of (seed, b) alone, cycling through: a planted
    sparse mixture X0 w; the same mixture shrunk by 0.6 (under sum_to_one = False the sum constraint is inactive); a genotype
    row of G divided by 2 (noise: several bounds active, cor_pred well below 1).  No column is constant."""
    X0 = t["X0"]
    M, K = X0.shape
    Gf = fill_missing(t["G"], X0)
    F = np.empty((M, B), order="F")
    for b in range(B):
        rng = np.random.default_rng([seed, b])
        w = np.zeros(K)
        support = rng.choice(K, size=min(K, 3), replace=False)
        w[support] = rng.dirichlet(np.ones(support.size) * 2.0)
        kind = b % 3
        F[:, b] = X0 @ w if kind == 0 else 0.6 * (X0 @ w) if kind == 1 else Gf[rng.integers(Gf.shape[0])] / 2.0
        assert F[:, b].max() > F[:, b].min()
    return F


def definition_d(t, F):
    """d = X'((P'f) o corr) of every column of F in numpy, K x B, with X = P'X0"""
    X = t["P"].T @ t["X0"]
    return X.T @ ((t["P"].T @ F) * t["corr"][:, None])


def corrcoef_reference(X0, F, w):
    """(cor_each: B x K, cor_pred: B) by np.corrcoef; a prediction without variance gives NaN"""
    B, K = w.shape
    each, pred = np.empty((B, K)), np.empty(B)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            each[b] = [np.corrcoef(X0[:, k], F[:, b])[0, 1] for k in range(K)]
            pred[b] = np.corrcoef(X0 @ w[b], F[:, b])[0, 1]
    return each, pred


def assert_correlations(got_each, got_pred, want_each, want_pred, what):
    """within 1e-10, NaN at the same places"""
    for got, want in ((got_each, want_each), (got_pred, want_pred)):
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
        ok = ~np.isnan(want)
        assert (np.abs(got[ok] - want[ok]) <= 1e-10).all(), (what, np.abs(got[ok] - want[ok]).max())


def proven_drops(w, steps):
    """a lower bound on the partial steps (a constraint leaving the active set) of one solve: the final active set has at
    most #zeros + 1 members, and steps = adds + drops, so drops >= (steps - #zeros - 1) / 2"""
    return (int(steps) - int((np.asarray(w) == 0).sum()) - 1) // 2


def twin_settled(solve, A, trials=3):
    """Which problems the statement itself determines to a tenth of the 1e-10 that cor_pred is held to: solve(A) -> the
    statement's results for the frequency columns / genotype rows A; it is run again on A (1 + 2^-53 u), u uniform in
    [-1, 1] — one rounding of its input, the size of the difference between two orders of summation — and a problem counts
    as settled when no trial moves its cor_pred by more than 1e-11.  Where cond(Dmat) is about 1e8 the minimiser is
    determined to about 1e-8 along the directions that Dmat hardly sees, and cor_pred = cor(X0 w, f) sees those directions:
    on such a problem two correct solvers differ by more than 1e-10 (measured on the sweep: 2.4e-10 on the columns of
    (19, 5), 3.5e-11 on (60, 10); 3e-15 wherever cond(Dmat) <= 1e6), so the statement's number is no reference there."""
    rng = np.random.default_rng(53)
    base = solve(A)["cor_pred"]
    ok = np.ones(base.size, dtype=bool)
    for _ in range(trials):
        cp = solve(A * (1.0 + 2.0 ** -53 * rng.uniform(-1.0, 1.0, size=A.shape)))["cor_pred"]
        both_nan = np.isnan(cp) & np.isnan(base)
        with np.errstate(invalid="ignore"):
            ok &= both_nan | (np.abs(cp - base) <= 1e-11)
    return ok
