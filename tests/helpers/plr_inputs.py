"""Inputs of the big_spLinReg / big_spLogReg tests (tests/test_plr_cpu.py, tests/test_gpu_plr.py): the example data decoded on
the host, columns 0 .. 1499, four folds fixed by a seeded draw, and the phenotypes."""
import os

import numpy as np

N_COL = 1500
PATH = dict(nlambda=60, nlam_min=15, n_abort=5)


def y01_of(golden_dir):
    return np.array([int(line.split()[5]) for line in open(os.path.join(golden_dir, "example.fam"))]) - 1.0


def example_case(orc, golden_dir, example_bed):
    """X: 517 x 1500 doubles (the example data has no missing value); fold: ids 0 .. 3; ylin: every 400th column plus
    noise; y01: the .fam phenotype; ystrong / y01strong: phenotypes that a few columns explain almost entirely (for the
    optimality check, whose path must keep improving on the validation fold); read-only"""
    full = orc.read_bed(example_bed, na_val=3).astype(np.float64)
    assert full.shape == (517, 4542) and not (full == 3).any()
    X = np.asfortranarray(full[:, :N_COL])
    n = X.shape[0]
    rng = np.random.default_rng(2025)
    fold = rng.permutation(np.arange(n) % 4).astype(np.int32)
    causal = np.arange(0, N_COL, 400)
    eff = np.array([0.6, -0.5, 0.4, 0.5])
    ylin = X[:, causal] @ eff + rng.standard_normal(n)
    strong = np.array([10, 150, 300, 450, 590])
    lin = (X[:, strong] - X[:, strong].mean(axis=0)) @ np.array([1.0, -0.8, 0.9, 0.7, -1.1])
    ystrong = lin + 0.3 * rng.standard_normal(n)
    y01strong = (rng.random(n) < 1 / (1 + np.exp(-2.0 * lin))).astype(np.float64)
    out = dict(X=X, full=full, fold=fold, ylin=ylin, y01=y01_of(golden_dir), ystrong=ystrong, y01strong=y01strong)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- seeded cases past the first turn of every loop of plr.hip (tests/test_gpu_plr_shapes.py) ---------------
#
# A case is a dict: codes (n x m uint8 calls 0 / 1 / 2 of a 2-bit image) or dense (a float matrix), X (the decoded float64
# matrix the statement takes), fold, K, ys (family -> phenotype), kw (the path's arguments, spelt as both the statement and
# big_spLinReg / big_spLogReg spell them), covar, pf_X, pf_covar, exact (the statement takes the column sums as exact integers:
# an image).  tests/test_plr_inputs_cpu.py runs the statement alone on
# every case in both summation orders and asserts the condition the case is named for, so a device test cannot pass
# without reaching its branch.

SEED = 101
SEED_WIDE = 102     # (at 101 a column below 1024 decides lambda_max of fold 0: the condition of case B fails)
FAMILIES = ("linear", "logistic")


def genotypes(rng, n, m):
    """binomial(2, maf) calls, maf ~ U(0.1, 0.5) per column"""
    maf = rng.uniform(0.1, 0.5, size=m)
    return rng.binomial(2, maf, size=(n, m)).astype(np.uint8)


def draw_fold(rng, n, K):
    return rng.permutation(np.arange(n) % K).astype(np.int32)


def both(lin):
    """the linear phenotype and the logistic one derived from it: 1 above its median"""
    return dict(linear=lin, logistic=(lin > np.median(lin)).astype(np.float64))


def _case(name, fold, K, ys, kw, codes=None, dense=None, covar=None, pf_X=None, pf_covar=None, exact=None):
    X = np.asfortranarray((codes if dense is None else dense).astype(np.float64))
    out = dict(name=name, codes=codes, dense=dense, X=X, fold=fold, K=K, ys=ys, kw=kw, covar=covar, pf_X=pf_X,
               pf_covar=pf_covar, exact=(dense is None) if exact is None else exact)
    for v in (codes, dense, X, fold, covar, pf_X, pf_covar) + tuple(ys.values()):
        if v is not None:
            v.setflags(write=False)
    return out


def ref_kw(case, family, **over):
    """the arguments of plr_ref.fit for a case (after X, y, fold, K)"""
    m = case["X"].shape[1]
    kw = dict(case["kw"], family=family, exact=case["exact"], covar=case["covar"])
    if case["pf_X"] is not None or case["pf_covar"] is not None:
        q = 0 if case["covar"] is None else case["covar"].shape[1]
        kw["pf"] = np.r_[np.ones(m) if case["pf_X"] is None else case["pf_X"],
                         np.zeros(q) if case["pf_covar"] is None else case["pf_covar"]]
    kw.update(over)
    return kw


def dev_kw(case, **over):
    """the arguments of big_spLinReg / big_spLogReg for a case (after X, y)"""
    kw = dict(case["kw"], ind_sets=case["fold"], covar_train=case["covar"], pf_X=case["pf_X"], pf_covar=case["pf_covar"])
    kw.update(over)
    return kw


def wide_matrix(seed=SEED_WIDE):
    """300 x 1200 calls, two folds, y = 0.5 x5 + 0.9 x1090 + noise: cases A and B"""
    rng = np.random.default_rng(seed)
    g = genotypes(rng, 300, 1200)
    fold = draw_fold(rng, 300, 2)
    lin = 0.5 * g[:, 5] + 0.9 * g[:, 1090] + rng.standard_normal(300)
    return g, fold, both(lin)


def case_active_set_across_1024(seed=SEED_WIDE):
    """A: alpha = 0.001 over twelve lambdas down to 1e-4 lambda_max: the active set of every chain goes from a few dozen
    columns to more than 1024 of the 1200 (compact's second turn with a carried base, the commit's count and copy loops
    past 1024 entries, a sweep over more than 1024 listed columns)"""
    g, fold, ys = wide_matrix(seed)
    return _case("A", fold, 2, ys, dict(alphas=[0.001], nlambda=12, lambda_min_ratio=1e-4, nlam_min=12, n_abort=12), codes=g)


def case_lambda_max_past_1024(seed=SEED_WIDE):
    """B: the same matrix at alpha = 1: column 1090 decides lambda_max in every chain (k_plr_lmax's second turn)"""
    g, fold, ys = wide_matrix(seed)
    return _case("B", fold, 2, ys, dict(alphas=[1.0], nlambda=10, nlam_min=4, n_abort=2), codes=g)


def lambda_max_below(case, family, chain, stop):
    """lambda_max of a chain restated in numpy over the columns < stop: max |x~' (y - ybar)| / (nt a pf) on the training
    rows (both families start from the mean, so g = y - ybar in both)"""
    k, a = chain % case["K"], case["kw"]["alphas"][chain // case["K"]]
    tr = case["fold"] != k
    Xt, y = case["X"][tr][:, :stop], case["ys"][family][tr]
    s = Xt.std(axis=0)
    z = ((Xt - Xt.mean(axis=0)) / np.where(s > 0, s, np.inf)).T @ (y - y.mean()) / tr.sum()
    return np.abs(z).max() / a


C_ORDERS = ([0.001, 0.002, 1.0], [1.0, 0.001, 0.002])


def case_chain_blocks(order, seed=SEED):
    """C: four folds x three alphas = twelve chains = a block of eight and a block of four in k_plr_scan; dfmax = 30 ends
    the two small alphas early ("Too many variables") while alpha = 1 walks the whole grid.  order 0: block 0 is all
    dead while block 1 runs; order 1: block 1 is all dead while block 0 is half dead"""
    rng = np.random.default_rng(seed)
    g = genotypes(rng, 300, 200)
    fold = draw_fold(rng, 300, 4)
    lin = 0.5 * g[:, 5] + 0.9 * g[:, 50] - 0.7 * g[:, 150] + rng.standard_normal(300)
    return _case("C%d" % order, fold, 4, both(lin),
                 dict(alphas=list(C_ORDERS[order]), nlambda=30, lambda_min_ratio=0.05, nlam_min=30, n_abort=30, dfmax=30), codes=g)


def correlated_matrix(seed=SEED):
    """300 x 40 calls, columns 1 and 2 copies of column 0 on 90 % of the rows, two folds: cases D, E and K"""
    rng = np.random.default_rng(seed)
    g = genotypes(rng, 300, 40)
    for j in (1, 2):
        same = rng.random(300) < 0.9
        g[same, j] = g[same, 0]
    fold = draw_fold(rng, 300, 2)
    return rng, g, fold


def case_max_iter(max_iter, seed=SEED):
    """D: eps = 1e-9 on three nearly collinear columns: every lambda after the start uses up max_iter passes, so the
    commit closes it on `iter_l >= max_iter` whether or not the scan added a column"""
    rng, g, fold = correlated_matrix(seed)
    lin = 1.0 * g[:, 0] - 0.8 * g[:, 1] + 0.6 * g[:, 2] + 0.3 * rng.standard_normal(300)
    return _case("D%d" % max_iter, fold, 2, both(lin),
                 dict(alphas=[1.0, 0.5], nlambda=10, lambda_min_ratio=0.05, nlam_min=10, n_abort=10, eps=1e-9,
                      max_iter=max_iter), codes=g)


def case_penalty_factors(seed=SEED):
    """E: pf_X ~ U(0.5, 2) with columns 3 and 17 unpenalised (flagged in k_plr_init: the start set), one covariate with
    penalty factor 1.5 (it enters through k_plr_flag at j >= m)"""
    rng, g, fold = correlated_matrix(seed)
    cov = rng.standard_normal((300, 1))
    pf = rng.uniform(0.5, 2.0, size=40)
    pf[[3, 17]] = 0.0
    lin = 1.0 * g[:, 0] - 0.8 * g[:, 1] + 0.6 * g[:, 2] + 0.5 * g[:, 3] + 0.8 * cov[:, 0] + 0.3 * rng.standard_normal(300)
    return _case("E", fold, 2, both(lin), dict(alphas=[1.0, 0.3], nlambda=15, nlam_min=5, n_abort=3), codes=g,
                 covar=np.asfortranarray(cov), pf_X=pf, pf_covar=np.array([1.5]))


def case_saturated():
    """F: the separable toy of tests/test_plr_cpu.py::test_messages: y = x0 > 0 ends "Model saturated" on every fold"""
    rng = np.random.default_rng(3)
    n = 120
    X = rng.standard_normal((n, 5))
    y = (X[:, 0] > 0).astype(np.float64)
    return _case("F", (np.arange(n) % 3).astype(np.int32), 3, dict(logistic=y),
                 dict(nlambda=100, lambda_min_ratio=1e-4, n_abort=100), dense=X)


G_ZERO_2BIT = [(j, c) for j in (4, 5, 6) for c in range(3)] + [(j, 1) for j in (7, 8, 9)]
G_ZERO_DENSE = G_ZERO_2BIT + [(10, c) for c in range(3)] + [(11, 2)] + [(12, c) for c in range(3)] + [(13, 0)]


def case_constant_columns(dense, seed=SEED):
    """G: 300 x 30, three folds.  Columns 4, 5, 6 are all 0, all 1, all 2; columns 7, 8, 9 are 0, 1, 2 on the training
    rows of fold 1 and vary inside fold 1.  dense: the same values as float64, with column 10 = 0.1 everywhere and
    column 11 = 0.1 outside fold 2, column 12 = 1 / 3 everywhere and column 13 = 1 / 3 outside fold 0.  The row-by-row
    mean of 200 times 0.1 is not 0.1, so the statement needs `lo == hi`; k_plr_stats' own tree (device_tree_sum) happens
    to return 0.1 exactly on these folds, and does not for 1 / 3: that column is the one on which the kernel needs it"""
    rng = np.random.default_rng(seed)
    g = genotypes(rng, 300, 30)
    fold = draw_fold(rng, 300, 3)
    for v, j in enumerate((4, 5, 6)):
        g[:, j] = v
    for v, j in enumerate((7, 8, 9)):
        g[:, j] = np.where(fold == 1, (np.arange(300) + v) % 3, v)
    lin = 0.8 * g[:, 0] - 0.6 * g[:, 1] + 0.5 * g[:, 20] + rng.standard_normal(300)
    kw = dict(nlambda=15, nlam_min=5, n_abort=3)
    if not dense:
        return _case("G 2-bit", fold, 3, both(lin), kw, codes=g)
    A = g.astype(np.float64)
    A[:, 10] = 0.1
    A[:, 11] = np.where(fold == 2, A[:, 11], 0.1)
    A[:, 12] = 1.0 / 3.0
    A[:, 13] = np.where(fold == 0, A[:, 13], 1.0 / 3.0)
    return _case("G dense", fold, 3, both(lin), kw, dense=A)


def device_tree_sum(v, threads=256):
    """the sum of v in the order of k_plr_stats (block_sum<., 256>): thread t adds the rows t, t + 256, ... in turn, a
    butterfly (offsets 32 .. 1) inside each wave of 64, then the waves in index order"""
    part = np.zeros(threads)
    for i in range(v.size):
        part[i % threads] = part[i % threads] + v[i]
    w = part.reshape(threads // 64, 64).copy()
    off = 32
    while off > 0:
        w[:, :off] = w[:, :off] + w[:, off:2 * off]
        off //= 2
    s = 0.0
    for k in range(threads // 64):
        s = s + w[k, 0]
    return s


def case_monomorphic(dense, seed=SEED):
    """H: 50 x 3, columns all 1, all 2, all 0, y noise: lambda_max = 0, a grid of zeros, nothing ever enters"""
    rng = np.random.default_rng(seed)
    g = np.repeat(np.array([[1, 2, 0]], dtype=np.uint8), 50, axis=0)
    fold = (np.arange(50) % 2).astype(np.int32)
    ys = dict(linear=rng.standard_normal(50))
    kw = dict(nlambda=6, nlam_min=2, n_abort=2)
    return _case("H dense", fold, 2, ys, kw, dense=g.astype(np.float64)) if dense else _case("H 2-bit", fold, 2, ys, kw, codes=g)


SMALL_SHAPES = ((5, 1), (37, 3), (64, 2), (65, 1))


def case_small(n, m, dense, seed=SEED):
    """I: fewer rows than a wave (5, 37), exactly one wave (64), one more (65); one column; column 0 is i mod 3.  dense:
    the same values as float32"""
    rng = np.random.default_rng(seed)
    g = genotypes(rng, n, m)
    g[:, 0] = np.arange(n) % 3
    fold = (np.arange(n) % 2).astype(np.int32)
    lin = g[:, 0] + 0.5 * rng.standard_normal(n)
    kw = dict(nlambda=8, nlam_min=3, n_abort=2, lambda_min_ratio=0.1)
    name = "I %d x %d %s" % (n, m, "float32" if dense else "2-bit")
    return _case(name, fold, 2, both(lin), kw, dense=g.astype(np.float32)) if dense else _case(name, fold, 2, both(lin), kw, codes=g)


def case_byte_selection(seed=SEED):
    """J: a 700 x 60 panel of CODE_DOSAGE grid indices k in -100 .. 100, an unsorted ind_train of 333 rows, every other
    column, two unpenalised covariates, three folds.  Returns (k, rows, cols, case); the case is over the selection, with
    `dense` the decoded sub-matrix (1 + 0.01 k as the table rounds it) and `exact` set, as for every image"""
    import dosage_inputs as dos
    rng = np.random.default_rng(seed)
    k = rng.integers(-100, 101, size=(700, 60)).astype(np.int8)
    rows = rng.permutation(700)[:333].astype(np.int64)
    cols = np.arange(0, 60, 2, dtype=np.int64)
    sub = np.asfortranarray(dos.CODE_DOSAGE[dos.dosage_bytes(k)][np.ix_(rows, cols)])
    cov = np.asfortranarray(rng.standard_normal((333, 2)))
    fold = draw_fold(rng, 333, 3)
    lin = sub[:, [1, 7, 20]] @ np.array([1.2, -1.0, 0.9]) + 0.7 * cov[:, 0] - 0.4 * cov[:, 1] + 0.5 * rng.standard_normal(333)
    case = _case("J", fold, 3, both(lin), dict(nlambda=20, nlam_min=6, n_abort=3), dense=sub, covar=cov, exact=True)
    return k, rows, cols, case
