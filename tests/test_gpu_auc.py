"""AUC / AUCBoot / big_prodMat / snp_grid_AUC / pcor on the device (csrc/auc.hip).  AUC is held to the O(n1 n0) definition in
numpy integers and the bootstrap replicates to the CPU statement (tests/native/auc_ref.cpp), both with array_equal: the
rule is exact integers and one division.  Independent of the header: the device's draws against a numpy restatement of
the resample rule, replicates against the definition on the resampled vectors, the statistics against numpy."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import auc_ref as ref  # noqa: E402
from test_impute_cpu import philox4x32_10  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture()
def batch(monkeypatch):
    def set_(v):
        if v is None:
            monkeypatch.delenv("BSN_AUC_BATCH", raising=False)
        else:
            monkeypatch.setenv("BSN_AUC_BATCH", str(v))
    set_(None)
    return set_


def scores(n, K, seed, kind="mixed"):
    """n x K: column j cycles through continuous values, a 3-value lattice, a 17-value lattice and values with +-0 / +-Inf"""
    rng = np.random.default_rng(seed)
    X = np.empty((n, K), order="F")
    for j in range(K):
        k = j % 4 if kind == "mixed" else kind
        if k == 0:
            X[:, j] = rng.normal(size=n)
        elif k == 1:
            X[:, j] = rng.integers(0, 3, n) - 1.0
        elif k == 2:
            X[:, j] = rng.integers(0, 17, n) / 4.0
        else:
            X[:, j] = rng.choice([-np.inf, np.inf, -0.0, 0.0, 1.5, -1.5, 2.5], n)
    return X


def target(n, seed, frac=0.4):
    rng = np.random.default_rng(seed + 1000)
    y = (rng.uniform(size=n) < frac).astype(np.int64)
    y[0], y[n - 1] = 0, 1
    return y


def definition(X, y):
    return np.array([ref.auc_definition(X[:, j], y) for j in range(X.shape[1])])


# ---- AUC -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,cap", [(2, 1, None), (257, 3, None), (1025, 70, 32), (5000, 3, None), (5000, 1, None)])
def test_auc_against_the_definition(ba, batch, n, K, cap):
    batch(cap)                       # K = 70 at 32 columns per batch: the column loop turns three times
    X, y = scores(n, K, n + K), target(n, n)
    got = ba.AUC(X, y)
    assert got.shape == (K,)
    assert np.array_equal(got, definition(X, y))
    assert np.array_equal(ba.AUC(X, y), got)                 # two calls, the same bytes
    assert ba.AUC(X[:, 0], y) == got[0]                      # a vector gives a float


def test_auc_tie_structures(ba, batch):
    n = 5000
    y = target(n, 5)
    lattice = scores(n, 2, 7, kind=1)                        # 3 values: tie groups span every tile border
    assert np.array_equal(ba.AUC(lattice, y), definition(lattice, y))
    distinct = np.random.default_rng(8).permutation(n).astype(np.float64)
    assert np.array_equal(ba.AUC(distinct, y), definition(distinct[:, None], y)[0])
    assert ba.AUC(np.full(n, 2.5), y) == 0.5
    assert ba.AUC(np.where(np.arange(n) % 2 == 0, -0.0, 0.0), y) == 0.5
    assert ba.AUC(np.array([0.0, 1.0]), [0, 1]) == 1.0 and ba.AUC(np.array([0.0, 1.0]), [1, 0]) == 0.0
    assert ba.AUC(distinct, y, digits=3) == np.round(ba.AUC(distinct, y), 3)


def test_auc_input_forms(ba, batch):
    n, K = 1025, 5
    X, y = scores(n, K, 21), target(n, 21)
    want = definition(X, y)
    big = np.full((n + 7, K), np.nan, order="F")             # leading dimension n + 7, NaN below
    big[:n] = X
    assert np.array_equal(ba.AUC(big[:n], y), want)
    X32 = np.asfortranarray(X.astype(np.float32))
    with np.errstate(invalid="ignore"):
        want32 = definition(X32.astype(np.float64), y)
    assert np.array_equal(ba.AUC(X32, y), want32)
    big32 = np.zeros((n + 7, K), dtype=np.float32, order="F")
    big32[:n] = X32
    assert np.array_equal(ba.AUC(big32[:n], y), want32)
    assert np.array_equal(ba.AUC(np.ascontiguousarray(X), y), want)      # row-major: copied once
    d = ba.DeviceArray.from_numpy(X)
    assert np.array_equal(ba.AUC(d, y), want)
    rows = np.sort(np.random.default_rng(2).choice(n, 400, replace=False))
    yr = target(400, 3)
    want_rows = definition(X[rows], yr)
    assert np.array_equal(ba.AUC(X, yr, ind_row=rows), want_rows)
    assert np.array_equal(ba.AUC(d, yr, ind_row=rows), want_rows)
    assert np.array_equal(ba.AUC(big[:n], yr, ind_row=rows[::-1]), definition(X[rows[::-1]], yr))
    d.free()


def test_auc_refusals(ba, batch):
    n = 300
    X, y = scores(n, 6, 4), target(n, 4)
    X[17, 4] = X[3, 5] = np.nan
    d = ba.DeviceArray.from_numpy(X)
    with pytest.raises(ba.BsnError, match=r"AUC: missing value \(NaN\) in 'pred', first in column 4"):
        ba.AUC(d, y)                                         # found on the device
    batch(2)
    with pytest.raises(ba.BsnError, match="first in column 4"):
        ba.AUC(d, y)
    with pytest.raises(ValueError, match="first in column 4"):
        ba.AUC(X, y)                                         # found on the host
    with pytest.raises(ValueError, match="'target' should hold 0 and 1 only"):
        ba.AUC(d, np.full(n, 2))
    with pytest.raises(ValueError, match="'target' should hold both classes"):
        ba.AUC(d, np.ones(n))
    d.free()


# ---- big_prodMat ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example(ba, orc, example_bed, golden_dir):
    gb = ba.bed(os.path.join(golden_dir, "example.bed"))
    G = ba.read_bed(gb, None, None).astype(np.float64)
    assert G.shape == (517, 4542) and G.min() >= 0          # the example data holds no missing value
    fbm = ba.FBM_code256(orc.fbm_from_bed(example_bed).bytes)
    return gb, fbm, G


@pytest.mark.parametrize("K", [1, 20])
def test_prodmat_against_numpy(ba, example, K):
    gb, fbm, G = example
    rng = np.random.default_rng(K)
    Ai = rng.integers(-3, 4, size=(G.shape[1], K)).astype(np.float64)
    for obj in (gb, fbm):
        assert np.array_equal(ba.big_prodMat(obj, Ai), G @ Ai)
    A = rng.normal(0, 0.1, size=(G.shape[1], K))
    A[:, K - 1] = np.nan                                     # a grid point that diverged
    want = G @ A
    fin = np.isfinite(want)
    # the bar of the kernel behind prod_and_rowSumsSq: tests/test_gpu_prs_tcrossprod.py:102, atol = 1e-9 max|ref|
    tol = 1e-9 * np.abs(want[fin]).max() if fin.any() else 0.0
    for obj in (gb, fbm):
        got = ba.big_prodMat(obj, A)
        assert np.isnan(got[:, K - 1]).all() and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.abs(got[fin] - want[fin]).max() <= tol if fin.any() else True
    ir = np.sort(rng.choice(G.shape[0], 200, replace=False))
    ic = np.sort(rng.choice(G.shape[1], 1000, replace=False))
    A2 = rng.normal(size=(ic.size, K))
    want = G[np.ix_(ir, ic)] @ A2
    for obj in (gb, fbm):
        got = ba.big_prodMat(obj, A2, ind_row=ir, ind_col=ic)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    center, scale = G[:, ic].mean(axis=0), G[:, ic].std(axis=0) + 0.5
    want = ((G[np.ix_(ir, ic)] - center) / scale) @ A2
    got = ba.big_prodMat(gb, A2, ind_row=ir, ind_col=ic, center=center, scale=scale)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    if K == 1:
        assert np.array_equal(ba.big_prodMat(gb, Ai[:, 0]), G @ Ai)       # a vector is one column


def test_prodmat_on_device_feeds_auc(ba, example, batch):
    gb, _, G = example
    rng = np.random.default_rng(9)
    A = rng.normal(0, 0.1, size=(G.shape[1], 6))
    y = target(G.shape[0], 9)
    host = ba.big_prodMat(gb, A)
    d = ba.big_prodMat(gb, A, on_device=True)
    assert isinstance(d, ba.DeviceArray) and (d.rows, d.cols) == host.shape
    assert np.array_equal(d.to_numpy(), host)
    got = ba.AUC(d, y)
    assert np.array_equal(got, definition(host, y))
    A[:, 2] = np.nan
    d2 = ba.big_prodMat(gb, A, on_device=True)
    with pytest.raises(ba.BsnError, match="first in column 2"):
        ba.AUC(d2, y)
    d.free(), d2.free()


# ---- snp_grid_AUC ----------------------------------------------------------------------------------------------------------
def test_grid_auc_against_sum_then_auc(ba, orc, example, golden_dir, batch):
    gb, fbm, G = example
    m = G.shape[1]
    rng = np.random.default_rng(6)
    CHR = np.repeat([1, 2, 3], [1514, 1514, 1514])           # three pseudo-chromosomes, as the vignette's 22
    POS = orc.read_bim(os.path.join(golden_dir, "example.bed"))[1]
    lpval = -np.log10(rng.uniform(size=m))
    betas = rng.normal(0, 0.1, m)
    keep = ba.snp_grid_clumping(fbm, CHR, POS, lpval, grid_thr_r2=(0.05, 0.8), grid_base_size=(100, 200))
    prs = ba.snp_grid_PRS(fbm, keep, betas, lpval, n_thr_lpS=7)
    assert prs.scores.dtype == np.float32
    s = prs.shape[1] // 3
    assert s == 4 * 7
    y = (G @ betas + rng.normal(0, 1.0, G.shape[0]) > np.median(G @ betas)).astype(np.int64)
    tab = ba.snp_grid_AUC(prs, y)
    sums = np.zeros((G.shape[0], s), order="F")
    for c in range(3):                                       # fp64, ascending chromosome order
        sums += prs.scores[:, c * s:(c + 1) * s].astype(np.float64)
    assert np.array_equal(tab["auc"], ba.AUC(sums, y))
    assert np.array_equal(tab["auc"], definition(sums, y))
    assert np.array_equal(tab["id"], np.repeat(np.arange(4), 7))
    assert np.array_equal(tab["thr_lp"], np.tile(prs.grid_lpS_thr, 4))
    for k in ("size", "thr_r2", "grp_num", "thr_imp"):
        assert np.array_equal(tab[k], np.repeat(keep.grid[k], 7))
    batch(5)
    assert np.array_equal(ba.snp_grid_AUC(prs, y)["auc"], tab["auc"])
    rows = np.arange(0, G.shape[0], 2)
    assert np.array_equal(ba.snp_grid_AUC(prs, y[rows], ind_row=rows)["auc"], definition(sums[rows], y[rows]))
    d = ba.DeviceArray.from_numpy(prs.scores.astype(np.float64))
    assert np.array_equal(ba.snp_grid_AUC(d, y, n_chr=3)["auc"], tab["auc"])
    d.free()


# ---- AUCBoot ---------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_values(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_boot_one_case(ba, batch):
    n, nboot = 6, 64
    X = scores(n, 2, 1)
    y = np.array([0, 0, 1, 0, 0, 0])
    r = ba.AUCBoot(X, y, nboot=nboot, seed=7)
    want = ref.boot(X, y, nboot, 7)
    assert same_values(r.replicates, want)
    nan = np.isnan(r.replicates[:, 0])
    assert 0.15 < nan.mean() < 0.55                          # (5/6)^6 = 0.335 of the resamples hold no case
    assert np.array_equal(nan, np.isnan(want[:, 0]))


def test_boot_against_the_twin(ba, batch):
    n, nboot = 300, 1000
    X, y = scores(n, 3, 31), target(n, 31)                   # three columns of different tie structure in one call
    r = ba.AUCBoot(X, y, nboot=nboot, seed=2 ** 40 + 5)
    assert r.shape == (3, 4) and r.replicates.shape == (nboot, 3) and r.seed == 2 ** 40 + 5
    assert same_values(r.replicates, ref.boot(X, y, nboot, 2 ** 40 + 5))
    batch(16)
    r16 = ba.AUCBoot(X, y, nboot=nboot, seed=2 ** 40 + 5)
    assert same_bits(r16.replicates, r.replicates) and same_bits(np.asarray(r16), np.asarray(r))
    batch(None)
    again = ba.AUCBoot(X, y, nboot=nboot, seed=2 ** 40 + 5)
    assert same_bits(again.replicates, r.replicates)
    other = ba.AUCBoot(X, y, nboot=nboot, seed=2 ** 40 + 6)
    assert not np.array_equal(other.replicates, r.replicates)
    # a vector, and the statistics against numpy on the replicates
    v = ba.AUCBoot(X[:, 0], y, nboot=nboot, seed=2 ** 40 + 5)
    assert v.shape == (4,) and same_bits(v.replicates[:, 0], r.replicates[:, 0])
    for j in range(3):
        rep = r.replicates[:, j]
        assert np.array_equal(np.asarray(r)[j], [rep.mean(), *np.quantile(rep, [0.025, 0.975]), rep.std(ddof=1)])
    assert np.array_equal(np.asarray(ba.AUCBoot(X, y, nboot=50, seed=1, digits=3)), np.round(np.asarray(ba.AUCBoot(X, y, nboot=50, seed=1)), 3))


def test_boot_workgroups_take_several_replicates(ba, batch):
    """more replicates than the 1 024 workgroups of a launch: a workgroup evaluates a histogram, clears it and fills it
    again for its next replicate — on a 3-value lattice that is the same 24 bytes every time"""
    n, nboot = 300, 2500
    X, y = scores(n, 2, 41), target(n, 41)
    r = ba.AUCBoot(X, y, nboot=nboot, seed=11)
    assert same_values(r.replicates, ref.boot(X, y, nboot, 11))
    assert same_bits(ba.AUCBoot(X, y, nboot=nboot, seed=11).replicates, r.replicates)


def test_boot_rows_above_65536(ba, batch):
    n, nboot = 70001, 64
    X, y = scores(n, 2, 77), target(n, 77)
    r = ba.AUCBoot(X, y, nboot=nboot, seed=3)
    assert same_values(r.replicates, ref.boot(X, y, nboot, 3))
    d = ba.DeviceArray.from_numpy(X)
    assert same_bits(ba.AUCBoot(d, y, nboot=nboot, seed=3).replicates, r.replicates)
    d.free()


def test_boot_independent_of_the_header(ba, batch):
    n = 1000
    X, y = scores(n, 2, 13), target(n, 13)
    seed = 2 ** 63 + 99
    r = ba.AUCBoot(X, y, nboot=8, seed=seed)
    for b in range(8):
        rows = ba.auc_boot_draws(n, b, seed)
        assert np.array_equal(rows, ref.philox_rows(philox4x32_10, n, b, seed))
        for j in range(2):
            assert r.replicates[b, j] == ref.auc_definition(X[rows, j], y[rows])
    rows = ba.auc_boot_draws(70001, 5, 1)
    assert np.array_equal(rows, ref.philox_rows(philox4x32_10, 70001, 5, 1)) and rows.max() > 65536


# ---- pcor ------------------------------------------------------------------------------------------------------------------
def pcor_numpy(X, y, Z, alpha=0.05):
    from statistics import NormalDist
    n = X.shape[0]
    D = np.ones((n, 1)) if Z is None else np.column_stack([np.ones(n), Z])
    c = D.shape[1] - 1
    ry = y - D @ np.linalg.lstsq(D, y, rcond=None)[0]
    out = np.empty((X.shape[1], 3))
    q = NormalDist().inv_cdf(1 - alpha / 2) / np.sqrt(n - c - 3)
    for j in range(X.shape[1]):
        rx = X[:, j] - D @ np.linalg.lstsq(D, X[:, j], rcond=None)[0]
        r = np.corrcoef(rx, ry)[0, 1]
        out[j] = r, np.tanh(np.arctanh(r) - q), np.tanh(np.arctanh(r) + q)
    return out


@pytest.mark.parametrize("c", [0, 3, 30])
def test_pcor_against_numpy(ba, c):
    """1e-11 absolute on r and both bounds: three fp64 sums of n products enter r; summed in different orders they differ
    by at most n 2^-53 = 5.6e-13 relative at n = 5000; 1e-11 leaves a factor of about six over the three together."""
    n, K = 5000, 5
    rng = np.random.default_rng(c)
    Z = rng.normal(size=(n, c)) if c else None
    y = rng.normal(size=n) + (Z[:, 0] if c else 0.0)
    X = rng.normal(size=(n, K)) + 0.3 * y[:, None]
    if c:
        X[:, 1] += 2.0 * Z[:, c - 1]
    X[:, 2] = 1e4 + rng.normal(size=n) + 0.1 * y            # a mean that dwarfs the spread
    got = ba.pcor(X, y, Z)
    want = pcor_numpy(X, y, Z)
    assert got.shape == (K, 3)
    print("pcor c=%d: max abs error %.3e" % (c, np.abs(got - want).max()))
    assert np.abs(got - want).max() <= 1e-11
    assert np.array_equal(ba.pcor(X, y, Z), got)             # two calls, the same bytes
    d = ba.DeviceArray.from_numpy(X)
    assert np.array_equal(ba.pcor(d, y, Z), got)
    d.free()
    assert np.array_equal(ba.pcor(X[:, 3], y, Z), got[3])
    wide = ba.pcor(X, y, Z, alpha=0.01)
    assert (wide[:, 1] < got[:, 1]).all() and (wide[:, 2] > got[:, 2]).all() and np.array_equal(wide[:, 0], got[:, 0])
    X32 = X[:, [0, 1, 3, 4]].astype(np.float32)
    assert np.abs(ba.pcor(X32, y, Z) - pcor_numpy(X32.astype(np.float64), y, Z)).max() <= 1e-11


def test_pcor_refusals(ba):
    rng = np.random.default_rng(1)
    n = 200
    X, y = rng.normal(size=(n, 2)), rng.normal(size=n)
    z = rng.normal(size=(n, 3))
    z[:, 2] = z[:, 0] + z[:, 1]
    with pytest.raises(ValueError, match=r"\[1, z\] is rank-deficient"):
        ba.pcor(X, y, z)
    Xn = X.copy()
    Xn[5, 1] = np.nan
    d = ba.DeviceArray.from_numpy(Xn)
    with pytest.raises(ValueError, match="non-finite value"):
        ba.pcor(d, y)                                        # seen in the device's sums
    d.free()
