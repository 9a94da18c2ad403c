"""snp_ldpred2_auto on the device against the CPU statement of src/ldpred2-auto.cpp (tests/native/ldpred2_auto_ref.cpp,
over the header the kernel is compiled from): every returned array bit for bit, on both kernel paths.  The LD matrix is
bed_cor of tests/golden/example.bed on the device; the summary statistics are those of test_gpu_ldpred2_grid.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import auto_statement  # noqa: E402
import ldpred2_auto_ref as ref  # noqa: E402
from auto_statement import equal_lists as _equal_lists  # noqa: E402
from auto_statement import same as _same  # noqa: E402
from scipy import sparse  # noqa: E402

P4 = [1e-4, 0.01, 0.3, 1.0]


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


@pytest.fixture(scope="module")
def full100(corr100):
    m2 = corr100.Dim[1]
    return ref.full_from_upper(corr100.p, corr100.i, corr100.x, m2) + (m2,)


@pytest.fixture(scope="module")
def sf100(ba, corr100):
    with ba.as_SFBM(corr100) as sf:
        yield sf


def _expected(ba, sf, full, df, vec_p_init, h2_init, seed, sub=None, **kw):
    """auto_statement.expected with the device's own mean LD score of the listed columns: an input to both sides"""
    mean_ld = float(np.mean(ba.ld_scores_sfbm(sf, sub)))
    return auto_statement.expected(full, df, mean_ld, vec_p_init, h2_init, seed, sub=sub, **kw)


def test_auto_equals_the_statement_and_seeds(ba, data, sf100, full100):
    df = data[2]
    m2 = full100[3]
    kw = dict(burn_in=20, num_iter=30, report_step=7)          # 4 report columns, 2 sweeps left over
    res = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=P4, seed=2024, **kw)
    want, raw = _expected(ba, sf100, full100, df, P4, 0.3, 2024, **kw)
    _same(res, want)
    for g, r in enumerate(res):
        assert r["sample_beta"].shape == (m2, 4) and r["path_p_est"].shape == (50,)
        assert np.isfinite(r["beta_est"]).all() and np.isfinite(r["path_alpha_est"]).all()
        assert r["seed"] == 2024 and r["stream"] == g and r["time"] > 0 and r["p_init"] == P4[g] and r["h2_init"] == 0.3
        assert "beta_est_sparse" not in r
        assert np.all(np.any(r["sample_beta"] != 0, axis=0))
    assert np.all(raw["moves"] > 0)
    # the same seed gives the same bits, another seed different ones
    again = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=P4, seed=2024, **kw)
    assert _equal_lists(again, res)
    other = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=P4, seed=2025, **kw)
    assert not any(np.array_equal(o["beta_est"], r["beta_est"]) for o, r in zip(other, res))
    # seed=None draws a fresh one, kept on the result
    a, b = (ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=[0.01, 0.3], burn_in=2, num_iter=3) for _ in range(2))
    assert a[0]["seed"] != b[0]["seed"] and a[0]["seed"] == a[1]["seed"]
    assert not np.array_equal(a[0]["beta_est"], b[0]["beta_est"])
    _same(a, _expected(ba, sf100, full100, df, [0.01, 0.3], 0.3, a[0]["seed"], burn_in=2, num_iter=3)[0])


def test_window_and_general_path_give_the_same_bits(ba, data, sf100, full100, monkeypatch):
    df = data[2]
    fits, rows = ref.envelope(full100[0], full100[1], full100[3])
    assert fits and rows <= ref.window_rows()              # by default this call takes the LDS window
    kw = dict(vec_p_init=P4, seed=7, burn_in=10, num_iter=20, report_step=6)
    win = ba.snp_ldpred2_auto(sf100, df, 0.3, **kw)
    monkeypatch.setenv("BSN_GIBBS_NO_WINDOW", "1")
    gen = ba.snp_ldpred2_auto(sf100, df, 0.3, **kw)
    monkeypatch.delenv("BSN_GIBBS_NO_WINDOW")
    win2 = ba.snp_ldpred2_auto(sf100, df, 0.3, **kw)
    assert _equal_lists(win, gen) and _equal_lists(win2, gen)
    _same(gen, _expected(ba, sf100, full100, df, P4, 0.3, 7, burn_in=10, num_iter=20, report_step=6)[0])


@pytest.mark.parametrize("flags", [dict(use_MLE=False), dict(shrink_corr=0.93), dict(allow_jump_sign=False),
                                   dict(alpha_bounds=(-1, -1)), dict(p_bounds=(0.02, 0.02)), dict(p_bounds=(1e-3, 0.05))],
                         ids=["no_mle", "shrink", "no_jump", "alpha_fixed", "p_fixed", "p_box"])
def test_each_flag_against_the_statement(ba, data, sf100, full100, flags):
    df = data[2]
    pv = [0.001, 0.03, 1.0]
    kw = dict(burn_in=10, num_iter=15, report_step=5)
    res = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=pv, seed=13, **kw, **flags)
    _same(res, _expected(ba, sf100, full100, df, pv, 0.3, 13, **kw, **flags)[0])
    for r in res:
        assert np.isfinite(r["beta_est"]).all()
        if flags.get("use_MLE") is False:
            assert np.isnan(r["path_alpha_est"]).all() and np.isnan(r["alpha_est"])
        if "alpha_bounds" in flags:
            assert np.all(r["path_alpha_est"] == -1)
        if flags.get("p_bounds") == (0.02, 0.02):
            assert np.all(r["path_p_est"] == 0.02)
        if flags.get("p_bounds") == (1e-3, 0.05):
            assert np.all((r["path_p_est"] >= 1e-3) & (r["path_p_est"] <= 0.05))


@pytest.mark.parametrize("m", [300, 257])
def test_empty_causal_set(ba, data, sf100, full100, m):
    """p_init at the lower bound of p on a few hundred variants: some sweeps end with nobody causal, the MLE keeps its
    parameters and rbeta is drawn at (1, 1 + m / mean_ld)"""
    df = data[2]
    sub = np.arange(1000, 1000 + m)
    dsub = {k: np.asarray(v)[sub] for k, v in df.items()}
    kw = dict(burn_in=10, num_iter=15, report_step=4)
    want, raw = _expected(ba, sf100, full100, dsub, [1e-5, 1e-5], 0.1, 5, sub=sub, **kw)
    assert np.any(raw["path_nb"] == 0) and np.all(raw["path_nb"] >= 0)
    res = ba.snp_ldpred2_auto(sf100, dsub, 0.1, vec_p_init=[1e-5, 1e-5], ind_corr=sub, seed=5, **kw)
    _same(res, want)


def test_subsets_via_ind_corr(ba, data, sf100, full100):
    df = data[2]
    fp, fi, fx, m2 = full100
    A = sparse.csc_matrix((fx, fi, fp), shape=(m2, m2))
    rng = np.random.default_rng(7)
    pv = [1.0, 0.1, 0.001]
    kw = dict(burn_in=10, num_iter=20, report_step=9)
    for sub in (np.sort(rng.choice(m2, 1500, replace=False)), rng.choice(m2, 1500, replace=False)):
        dsub = {k: np.asarray(v)[sub] for k, v in df.items()}
        res = ba.snp_ldpred2_auto(sf100, dsub, 0.3, vec_p_init=pv, ind_corr=sub, seed=11, **kw)
        _same(res, _expected(ba, sf100, full100, dsub, pv, 0.3, 11, sub=sub, **kw)[0])
        # auto(corr[sub, sub]) == auto(corr, ind.corr = sub) (test-8-LDpred2.R:266-287), here bit for bit
        res_sub = ba.snp_ldpred2_auto(A[sub][:, sub], dsub, 0.3, vec_p_init=pv, seed=11, **kw)
        assert _equal_lists(res_sub, res)


def test_sample_beta_identity(ba, data, sf100, full100):
    """test-8-LDpred2.R:105-106: with shrink_corr = 1 each reported column x has x' corr x == path_h2_est at its sweep,
    wherever the path is above the 1e-3 floor; 1.5e-8 is the tolerance of the reference's expect_equal"""
    df = data[2]
    fp, fi, fx, m2 = full100
    A = sparse.csc_matrix((fx, fi, fp), shape=(m2, m2))
    burn_in, num_iter, step = 20, 30, 7
    res = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=[0.001, 0.05, 1.0], seed=3, burn_in=burn_in, num_iter=num_iter,
                              report_step=step, shrink_corr=1)
    checked = 0
    for r in res:
        for c in range(num_iter // step):
            x = r["sample_beta"][:, c]
            h2 = r["path_h2_est"][burn_in + (c + 1) * step - 1]
            if h2 > 1e-3:
                assert abs(x @ (A @ x) - h2) <= 1.5e-8 * abs(h2)
                checked += 1
    assert checked >= 8


def test_sparse_follow_up(ba, data, sf100):
    """beta_est_sparse is snp_ldpred2_grid by hand at the chain's h2_est and p_est, sparse, on the stream | 2^63: bit for bit"""
    df = data[2]
    pv = [0.3, 0.005]
    res = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=pv, seed=21, burn_in=20, num_iter=30, sparse=True, stream=[4, 9])
    for r, st in zip(res, (4, 9)):
        gp = {"p": [r["p_est"]], "h2": [r["h2_est"]], "sparse": [True], "stream": np.array([st | 2 ** 63], dtype=np.uint64)}
        by_hand = np.asarray(ba.snp_ldpred2_grid(sf100, df, gp, burn_in=50, num_iter=100, seed=21))[:, 0]
        assert np.array_equal(r["beta_est_sparse"], by_hand)
        assert np.mean(r["beta_est_sparse"] == 0) > 0.5 and not np.any(r["beta_est"] == 0)


def test_stream_ids_make_chains_independent_of_the_call(ba, data, sf100):
    df = data[2]
    pv = np.array([1e-4, 0.003, 0.01, 0.1, 0.3, 1.0])
    kw = dict(seed=5, burn_in=5, num_iter=10, report_step=4)
    base = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=pv, **kw)
    perm = np.random.default_rng(3).permutation(pv.size)
    res = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=pv[perm], stream=perm, **kw)
    assert _equal_lists(res, [base[g] for g in perm])
    pick = np.array([4, 1])
    res = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=pv[pick], stream=pick, **kw)
    assert _equal_lists(res, [base[g] for g in pick])
    # without its ids the sub-list is another set of chains
    res = ba.snp_ldpred2_auto(sf100, df, 0.3, vec_p_init=pv[pick], **kw)
    assert not np.array_equal(res[0]["beta_est"], base[4]["beta_est"])


def test_divergence_gives_the_statements_nan_pattern(ba):
    """The size = 500 matrix with h2_init = 30 does not diverge under auto (found with the statement on the host: h2
    follows cur_h2_est after the first sweep), so the second candidate: 0.9 on the first two off-diagonals, m2 = 200, not
    positive definite.  Without the MLE the chains from p_init 0.01 and 0.3 cross gap > gap0 in their first sweep and
    those from 1e-4 and 1 stay finite; with it every chain stops after a few sweeps, its path finite up to there."""
    m2 = 200
    A = sparse.csc_matrix(sparse.diags([np.full(m2 - 2, 0.9), np.full(m2 - 1, 0.9), np.ones(m2), np.full(m2 - 1, 0.9),
                                        np.full(m2 - 2, 0.9)], [-2, -1, 0, 1, 2]))
    full = ref.full_csc(A) + (m2,)
    rng = np.random.default_rng(17)
    df = {"beta": rng.normal(0, 0.05, m2), "beta_se": np.full(m2, 0.03), "n_eff": np.full(m2, 1500.0)}
    kw = dict(burn_in=20, num_iter=30, report_step=7)
    with ba.as_SFBM(A) as sf:
        want, raw = _expected(ba, sf, full, df, P4, 0.3, 1, use_MLE=False, **kw)
        nan_chain = np.array([np.isnan(w["beta_est"]).all() for w in want])
        assert nan_chain.any() and not nan_chain.all()                       # checked on the host, before the device runs
        res = ba.snp_ldpred2_auto(sf, df, 0.3, vec_p_init=P4, seed=1, use_MLE=False, sparse=True, **kw)
        _same(res, want)
        for r, bad in zip(res, nan_chain):
            assert np.isnan(r["beta_est"]).all() == bad and np.isnan(r["postp_est"]).all() == bad
            assert np.isnan(r["h2_est"]) == bad and np.isnan(r["path_p_est"][-1]) == bad
            assert ("beta_est_sparse" in r) == (not bad)
        # with the MLE: finite path entries, then NaN from the sweep on at which the chain stopped
        want, raw = _expected(ba, sf, full, df, P4, 0.3, 1, **kw)
        stopped = (raw["path_nb"] >= 0).sum(axis=0)
        assert np.any((stopped > 0) & (stopped < 50))
        res = ba.snp_ldpred2_auto(sf, df, 0.3, vec_p_init=P4, seed=1, **kw)
        _same(res, want)
        for g, r in enumerate(res):
            assert np.isfinite(r["path_h2_est"][:stopped[g]]).all() and np.isnan(r["path_h2_est"][stopped[g]:]).all()
            assert np.all(r["sample_beta"] == 0) or stopped[g] > 26


def test_argument_errors_come_before_device_work(ba, data, sf100):
    df = data[2]
    m2 = sf100.ncol
    with pytest.raises(ValueError, match="'df_beta' should have element 'beta'."):
        ba.snp_ldpred2_auto(sf100, {k: v for k, v in df.items() if k != "beta"}, 0.3)
    with pytest.raises(ValueError, match="'h2_init' should have only positive values."):
        ba.snp_ldpred2_auto(sf100, df, -0.1)
    with pytest.raises(ValueError, match="Arguments should have the same length"):
        ba.snp_ldpred2_auto(sf100, {k: np.asarray(v)[:-1] for k, v in df.items()}, 0.3)
    with pytest.raises(ValueError, match="ind.corr %in% cols_along"):
        ba.snp_ldpred2_auto(sf100, df, 0.3, ind_corr=np.arange(1, m2 + 1))
    with pytest.raises(ValueError, match="'report_step' should be at least 1."):
        ba.snp_ldpred2_auto(sf100, df, 0.3, report_step=0)
    with pytest.raises(ValueError, match="below 2\\^30"):
        ba.snp_ldpred2_auto(sf100, df, 0.3, burn_in=2 ** 30 - 100, num_iter=100)
    # the library's own checks, through the C entry
    import ctypes as C
    from bigsnpr_amd import _lib
    z = np.zeros(m2)
    f64p = C.POINTER(C.c_double)
    p = z.ctypes.data_as(f64p)

    def call(h2_init=0.3, burn_in=5, num_iter=5, report_step=6):
        rc = _lib.load().bsn_ldpred2_auto(sf100.handle, p, p, p, m2, None, p, None, 1, h2_init, burn_in, num_iter, report_step, 0,
                                          1.0, 1, 1e-5, 1.0, -0.5, 1.5, 1.0, 1, p, p, p, p, p, p, p, None)
        assert rc != 0
        return _lib.load().bsn_last_error().decode()

    assert call(h2_init=0.0) == "'h2_init' should have only positive values."
    assert call(report_step=0) == "'report_step' should be at least 1."
    assert "below 2^30" in call(burn_in=2 ** 30 - 5, num_iter=5)
