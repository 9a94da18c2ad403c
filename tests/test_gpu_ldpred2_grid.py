"""snp_ldpred2_grid on the device against the CPU statement of src/ldpred2.cpp and src/ldpred2-sampling.cpp
(tests/native/ldpred2_ref.cpp, over the header the kernel is compiled from): bit for bit, on both kernel paths.  The LD
matrix is bed_cor of tests/golden/example.bed on the device; the summary statistics are those of test_gpu_lassosum2.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import ldpred2_ref as ref  # noqa: E402
from scipy import sparse  # noqa: E402

# the reference's grid (test-8-LDpred2.R:51-56): p = signif(seq_log(1e-3, 1, 7), 1) x sparse off / on
P7 = [0.001, 0.003, 0.01, 0.03, 0.1, 0.3, 1.0]
GRID14 = {"p": np.tile(P7, 2), "h2": np.full(14, 0.3), "sparse": np.repeat([False, True], 7)}


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def data(ba, golden_dir):
    gb = ba.bed(os.path.join(golden_dir, "example.bed"))
    G = ba.read_bed(gb, None, None).astype(np.float64)          # n x m, no missing values in this file
    keep = np.nonzero(G.std(axis=0) > 0)[0]
    G = G[:, keep]
    n, m = G.shape
    rng = np.random.default_rng(42)
    Z = (G - G.mean(axis=0)) / G.std(axis=0)
    b = np.where(rng.random(m) < 0.02, rng.normal(0, 0.3, m), 0.0)
    y = Z @ b + rng.normal(0, 1, n)
    gc = G - G.mean(axis=0)
    yc = y - y.mean()
    sxx = (gc * gc).sum(axis=0)
    beta = gc.T @ yc / sxx
    resid = ((yc[:, None] - gc * beta) ** 2).sum(axis=0) / (n - 2)
    df = {"beta": beta, "beta_se": np.sqrt(resid / sxx),
          "n_eff": np.round(n * rng.uniform(0.8, 1.0, m))}
    return gb, keep, df


@pytest.fixture(scope="module")
def corr100(ba, data):
    gb, keep, _ = data
    return ba.bed_cor(gb, ind_col=keep, size=100)


def _inputs(df, sub=None):
    take = (lambda a: np.asarray(a)) if sub is None else (lambda a: np.asarray(a)[sub])
    beta, se, n = take(df["beta"]), take(df["beta_se"]), take(df["n_eff"])
    scale = np.sqrt(n * se ** 2 + beta ** 2)
    return scale, beta / scale, n


def _full(corr):
    m2 = corr.Dim[1]
    return ref.full_from_upper(corr.p, corr.i, corr.x, m2) + (m2,)


def _expected(full, df, gp, seed, sub=None, stream=None, burn_in=50, num_iter=100):
    """the statement on the full columns, scaled back as R/LDpred2.R:139 does"""
    fp, fi, fx, m2 = full
    scale, bh, n = _inputs(df, None if sub is None else sub)
    beta, moves, _ = ref.grid(fp, fi, fx, m2, bh, n, gp["h2"], gp["p"], gp["sparse"], ind_sub=sub, stream=stream,
                              burn_in=burn_in, num_iter=num_iter, seed=seed, nthreads=16)
    return beta * scale[:, None]


def _same(res, want):
    assert res.shape == want.shape
    assert np.array_equal(np.asarray(res), want, equal_nan=True)


def test_reference_grid_equals_the_statement_and_seeds(ba, data, corr100):
    df = data[2]
    with ba.as_SFBM(corr100) as sf:
        res = ba.snp_ldpred2_grid(sf, df, GRID14, seed=2024)
        assert res.shape == (corr100.Dim[1], 14) and res.seed == 2024
        _same(res, _expected(_full(corr100), df, GRID14, 2024))
        assert np.isfinite(np.asarray(res)).all()
        assert np.all(res.grid_param["time"] > 0)
        assert not np.any(np.asarray(res)[:, :7] == 0) and np.mean(np.asarray(res)[:, 7 + 2] == 0) > 0.5
        # the same seed gives the same bits, another seed different ones
        again = ba.snp_ldpred2_grid(sf, df, GRID14, seed=2024)
        assert np.array_equal(np.asarray(again), np.asarray(res))
        other = ba.snp_ldpred2_grid(sf, df, GRID14, seed=2025, burn_in=5, num_iter=5)
        base = ba.snp_ldpred2_grid(sf, df, GRID14, seed=2024, burn_in=5, num_iter=5)
        assert not np.any(np.all(np.asarray(other) == np.asarray(base), axis=0))
        # seed=None draws a fresh one, kept on the result
        a, b = (ba.snp_ldpred2_grid(sf, df, GRID14, burn_in=2, num_iter=2) for _ in range(2))
        assert a.seed != b.seed and not np.array_equal(np.asarray(a), np.asarray(b))
        _same(a, _expected(_full(corr100), df, GRID14, a.seed, burn_in=2, num_iter=2))


def test_window_and_general_path_give_the_same_bits(ba, data, corr100, monkeypatch):
    df = data[2]
    full = _full(corr100)
    fits, rows = ref.envelope(full[0], full[1], full[3])
    assert fits and rows <= ref.window_rows()              # by default this call takes the LDS window
    with ba.as_SFBM(corr100) as sf:
        win = ba.snp_ldpred2_grid(sf, df, GRID14, seed=7, burn_in=10, num_iter=20)
        monkeypatch.setenv("BSN_GIBBS_NO_WINDOW", "1")
        gen = ba.snp_ldpred2_grid(sf, df, GRID14, seed=7, burn_in=10, num_iter=20)
        smp_gen = ba.snp_ldpred2_grid(sf, df, {"p": [0.03], "h2": [0.3], "sparse": [True]}, seed=7, burn_in=10, num_iter=20,
                                      return_sampling_betas=True)
        monkeypatch.delenv("BSN_GIBBS_NO_WINDOW")
        smp_win = ba.snp_ldpred2_grid(sf, df, {"p": [0.03], "h2": [0.3], "sparse": [True]}, seed=7, burn_in=10, num_iter=20,
                                      return_sampling_betas=True)
        win2 = ba.snp_ldpred2_grid(sf, df, GRID14, seed=7, burn_in=10, num_iter=20)
    assert np.array_equal(np.asarray(win), np.asarray(gen), equal_nan=True)
    assert np.array_equal(np.asarray(win2), np.asarray(gen), equal_nan=True)
    assert np.array_equal(np.asarray(smp_win), np.asarray(smp_gen))
    _same(gen, _expected(full, df, GRID14, 7, burn_in=10, num_iter=20))


def test_subsets_via_ind_corr(ba, data, corr100):
    df = data[2]
    full = _full(corr100)
    fp, fi, fx, m2 = full
    A = sparse.csc_matrix((fx, fi, fp), shape=(m2, m2))
    rng = np.random.default_rng(7)
    gp = {"p": np.array([1.0, 0.1, 0.01, 0.01]), "h2": np.full(4, 0.3), "sparse": np.array([False, False, False, True])}
    with ba.as_SFBM(corr100) as sf:
        for sub in (np.sort(rng.choice(m2, 1500, replace=False)), rng.choice(m2, 1500, replace=False)):
            dsub = {k: np.asarray(v)[sub] for k, v in df.items()}
            res = ba.snp_ldpred2_grid(sf, dsub, gp, ind_corr=sub, seed=11, burn_in=10, num_iter=20)
            _same(res, _expected(full, df, gp, 11, sub=sub, burn_in=10, num_iter=20))
            # ldpred2(corr[sub, sub]) == ldpred2(corr, ind.corr = sub) (test-8-LDpred2.R:266-287), here bit for bit
            res_sub = ba.snp_ldpred2_grid(A[sub][:, sub], dsub, gp, seed=11, burn_in=10, num_iter=20)
            assert np.array_equal(np.asarray(res_sub), np.asarray(res), equal_nan=True)


def test_stream_ids_make_chains_independent_of_the_call(ba, data, corr100):
    df = data[2]
    with ba.as_SFBM(corr100) as sf:
        base = np.asarray(ba.snp_ldpred2_grid(sf, df, GRID14, seed=5, burn_in=5, num_iter=10))
        perm = np.random.default_rng(3).permutation(14)
        gp = {k: np.asarray(v)[perm] for k, v in GRID14.items()}
        gp["stream"] = perm
        res = ba.snp_ldpred2_grid(sf, df, gp, seed=5, burn_in=5, num_iter=10)
        assert np.array_equal(np.asarray(res), base[:, perm])
        pick = np.array([12, 3, 6])
        gp = {k: np.asarray(v)[pick] for k, v in GRID14.items()}
        gp["stream"] = pick
        res = ba.snp_ldpred2_grid(sf, df, gp, seed=5, burn_in=5, num_iter=10)
        assert np.array_equal(np.asarray(res), base[:, pick])
        # without its ids the sub-grid is another set of chains
        del gp["stream"]
        res = ba.snp_ldpred2_grid(sf, df, gp, seed=5, burn_in=5, num_iter=10)
        assert not np.array_equal(np.asarray(res), base[:, pick])


def test_sampling_betas_equal_the_statement(ba, data, corr100):
    df = data[2]
    fp, fi, fx, m2 = _full(corr100)
    scale, bh, n = _inputs(df)
    for sp, p in ((False, 0.01), (True, 0.1)):
        gp = {"p": [p], "h2": [0.3], "sparse": [sp], "stream": [4]}
        res = ba.snp_ldpred2_grid(corr100, df, gp, seed=31, burn_in=10, num_iter=25, return_sampling_betas=True)
        assert res.shape == (m2, 25)
        want, _ = ref.sampling(fp, fi, fx, m2, bh, n, 0.3, p, sp, stream=4, burn_in=10, num_iter=25, seed=31)
        _same(res, want * scale[:, None])
        assert np.any(np.asarray(res)[:, -1] != 0)


def test_every_input_form_gives_the_same_bits(ba, data):
    gb, keep, df = data
    corr = ba.bed_cor(gb, ind_col=keep, size=60)
    fp, fi, fx, m2 = _full(corr)
    forms = [corr,                                                        # CorResult (upper, expanded on the device)
             corr.tocsc(),                                                # scipy, upper triangle
             sparse.csc_matrix((fx, fi, fp), shape=(m2, m2)),             # scipy, full columns
             ba.SFBM(fp, fi, fx, m2, False),                              # full columns given directly
             ba.SFBM(corr.p, corr.i, corr.x, m2, True)]
    gp = {"p": [1.0, 0.01], "h2": [0.3, 0.2], "sparse": [False, True]}
    outs = [ba.snp_ldpred2_grid(f, df, gp, seed=3, burn_in=5, num_iter=10) for f in forms]
    for o in outs[1:]:
        assert np.array_equal(np.asarray(o), np.asarray(outs[0]), equal_nan=True)
    _same(outs[0], _expected((fp, fi, fx, m2), df, gp, 3, burn_in=5, num_iter=10))
    for f in forms[3:]:
        f.close()


def test_divergence_gives_the_statements_nan_columns(ba, data):
    """a window of 500 variants over 517 samples is far from positive definite; with h2 inflated to 30 the p = 1 chain
    crosses gap > gap0 within a few sweeps (found with the statement on the host), the h2 = 0.3 chains do not"""
    gb, keep, df = data
    corr = ba.bed_cor(gb, ind_col=keep, size=500)
    gp = {"p": [1.0, 1.0, 0.01, 1.0, 0.01], "h2": [0.3, 30.0, 30.0, 100.0, 0.3], "sparse": [False, False, False, True, True]}
    res = ba.snp_ldpred2_grid(corr, df, gp, seed=1, burn_in=10, num_iter=10)
    want = _expected(_full(corr), df, gp, 1, burn_in=10, num_iter=10)
    nan_cols = np.isnan(want).all(axis=0)
    assert nan_cols.any() and not nan_cols.all()
    assert np.array_equal(np.isnan(np.asarray(res)).all(axis=0), nan_cols)
    _same(res, want)


def test_window_limit(ba):
    """m = 20 000 columns with a few entries each, one of them `half` rows from the diagonal: an envelope of 2 half + 64
    rows.  One half nearly fills the LDS window's budget, the other exceeds it and the host rule takes the general path;
    both equal the statement."""
    m2 = 20000
    W = ref.window_rows()
    rng = np.random.default_rng(17)
    df = {"beta": rng.normal(0, 0.05, m2), "beta_se": np.full(m2, 0.03), "n_eff": np.full(m2, 1500.0)}
    gp = {"p": [1.0, 0.05, 0.01], "h2": [0.2, 0.2, 0.2], "sparse": [False, False, True]}
    for half, fits in ((W // 2 - 40, True), (W // 2, False)):
        d = np.arange(m2 - half)
        far = sparse.coo_matrix((rng.uniform(-0.05, 0.05, d.size), (d, d + half)), shape=(m2, m2))
        near = sparse.diags([rng.uniform(-0.3, 0.3, m2 - 1)], [1])
        up = sparse.csc_matrix(far + near)
        A = sparse.csc_matrix(up + up.T + sparse.identity(m2))
        fp, fi, fx = ref.full_csc(A)
        got_fits, rows = ref.envelope(fp, fi, m2)
        assert got_fits == fits and rows == 2 * half + 64
        res = ba.snp_ldpred2_grid(A, df, gp, seed=9, burn_in=10, num_iter=20)
        want = _expected((fp, fi, fx, m2), df, gp, 9, burn_in=10, num_iter=20)
        _same(res, want)
        assert np.isfinite(want).all()
