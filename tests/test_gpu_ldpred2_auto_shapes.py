"""snp_ldpred2_auto (k_ldpred2_auto and run_auto of bigsnpr_amd/csrc/sparse_ld.hip) where its loops take a second turn or
none at all: columns longer than one round of add_column on both paths with a ring that wraps, systems of fewer
coordinates than one block of 64 and the sizes next to it, columns that store nothing, a causal set on both sides of
the stride of the epilogue's loops, the largest LDS window and the first envelope above it, and the report columns at
their edges.  The inputs are synthetic and seeded (tests/helpers/sfbm_inputs.py); tests/test_sfbm_inputs_cpu.py proves
without a GPU, against the constants read from the source, that each of them crosses its threshold.

The reference is the CPU statement tests/native/ldpred2_auto_ref.cpp (tests/helpers/auto_statement.py): every returned
array and scalar bit for bit, no tolerance anywhere.  The mean LD score is an input to both sides and comes from
ld_scores_sfbm on the same handle."""
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
import sfbm_inputs as si  # noqa: E402
from auto_statement import equal_lists, same  # noqa: E402

P4 = [1e-4, 0.01, 0.3, 1.0]


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def K():
    return si.kernel_constants()


def _expected(ba, sf, A, df, sub, kw, seed=si.AUTO_SEED):
    mean_ld = float(np.mean(ba.ld_scores_sfbm(sf, sub)))
    return auto_statement.expected(si.full_of(A), df, mean_ld, seed=seed, sub=sub, **kw)


def _finite(want):
    return all(np.isfinite(w[k]).all() for w in want for k in auto_statement.ARRAYS + auto_statement.SCALARS)


def _takes_window(A, sub):
    fp, fi, _ = si.csc_arrays(A)
    fits, rows = ref.envelope(fp, fi, A.shape[0], sub)
    return fits, rows


def _both_paths(ba, sf, df, sub, kw, monkeypatch, seed=si.AUTO_SEED):
    """the call as it is (the LDS window, for an ascending selection that fits) and on the general path"""
    win = ba.snp_ldpred2_auto(sf, df, ind_corr=sub, seed=seed, **kw)
    monkeypatch.setenv("BSN_GIBBS_NO_WINDOW", "1")
    gen = ba.snp_ldpred2_auto(sf, df, ind_corr=sub, seed=seed, **kw)
    monkeypatch.delenv("BSN_GIBBS_NO_WINDOW")
    return win, gen


# ---- 1. second round of add_column, a ring that wraps ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide(ba):
    A = si.wide_band()
    with ba.as_SFBM(A) as sf:
        yield A, sf


@pytest.mark.parametrize("case", [0, 1, 2], ids=["whole", "ascending", "unsorted"])
def test_wide_band_second_round(ba, K, wide, case, monkeypatch):
    A, sf = wide
    name, sub, df, ascending = si.wide_auto_cases(A)[case]
    L = np.diff(A.indptr)
    assert (L if sub is None else L[sub]).max() > K["kGibbsThreads"] * K["kGibbsAxpy"]
    fits, rows = _takes_window(A, sub)
    assert fits == ascending and (not fits or rows < A.shape[0])
    want, raw = _expected(ba, sf, A, df, sub, si.AUTO_WIDE)
    assert _finite(want) and np.all(raw["moves"] > 0)                  # checked on the host, before the device runs
    if ascending:
        win, gen = _both_paths(ba, sf, df, sub, si.AUTO_WIDE, monkeypatch)
        assert equal_lists(win, gen)
        same(win, want)
        same(gen, want)
    else:
        same(ba.snp_ldpred2_auto(sf, df, ind_corr=sub, seed=si.AUTO_SEED, **si.AUTO_WIDE), want)


# ---- 2. fewer coordinates than a block of 64, one block, just above -------------------------------------------------------------

@pytest.mark.parametrize("m", si.SMALL_M)
def test_small_systems(ba, m, monkeypatch):
    for name, A, sub, df in si.small_cases(m):
        with ba.as_SFBM(A) as sf:
            assert sf.ncol == (m if sub is None else si.SMALL_M2)
            want, raw = _expected(ba, sf, A, df, sub, si.AUTO_SMALL)
            assert _finite(want) and np.all(raw["moves"] > 0), name
            fits, _ = _takes_window(A, sub)
            assert fits == (name != "shuffled" or m == 1), name          # one position is in ascending order however shuffled
            if fits:
                win, gen = _both_paths(ba, sf, df, sub, si.AUTO_SMALL, monkeypatch)
                assert equal_lists(win, gen), name
                runs = (win, gen)
            else:
                runs = (ba.snp_ldpred2_auto(sf, df, ind_corr=sub, seed=si.AUTO_SEED, **si.AUTO_SMALL),)
            for res in runs:
                same(res, want)
                for r in res:
                    assert r["beta_est"].shape == (m,) and r["sample_beta"].shape == (m, 2), name
                    if sub is not None and si.EMPTY in sub:
                        # the column stores nothing: its dot product stays 0 and shrink_corr is 1, so every sweep adds an exact 0
                        at = int(np.nonzero(np.asarray(sub) == si.EMPTY)[0][0])
                        assert r["corr_est"][at] == 0, name


# ---- 3. a causal set on both sides of one stride of the epilogue's loops --------------------------------------------------------

def test_causal_set_straddles_one_stride(ba, K):
    A, df = si.straddle_case()
    stride = K["kGibbsThreads"]
    with ba.as_SFBM(A) as sf:
        want, raw = _expected(ba, sf, A, df, None, si.STRADDLE)
        nb = raw["path_nb"][:, 0]
        print("sweeps with fewer than %d causal: %d, with %d: %d, with more: %d" % (stride, np.sum(nb < stride), stride,
                                                                                    np.sum(nb == stride), np.sum(nb > stride)))
        assert nb.min() >= 0 and np.any(nb < stride) and np.any(nb == stride) and np.any(nb > stride)
        assert _finite(want)
        res = ba.snp_ldpred2_auto(sf, df, seed=si.AUTO_SEED, **si.STRADDLE)
        same(res, want)
        assert res[0]["sample_beta"].shape == (si.STRADDLE_M, si.STRADDLE["num_iter"])
        # every report column holds the causal set of its sweep: as many non-zero rows as path_nb says
        burn_in = si.STRADDLE["burn_in"]
        assert np.array_equal(np.count_nonzero(res[0]["sample_beta"], axis=0), nb[burn_in:])


# ---- 4. the largest LDS window and the first envelope above it --------------------------------------------------------------------

def test_window_limit(ba):
    """The fitting matrix asks for every ring row the host rule grants (128 KiB of dynamic LDS on top of the kernel's static
    LDS): the launch has to be accepted.  The other one is 16 rows above and takes the general path by the host rule."""
    W = ref.window_rows()
    for half, fits, A, df in si.window_limit_cases(W):
        got_fits, rows = _takes_window(A, None)
        assert got_fits == fits and rows == 2 * half + 64 and (not fits or -(-rows // 64) * 64 == W)
        with ba.as_SFBM(A) as sf:
            want, raw = _expected(ba, sf, A, df, None, si.WINDOW_LIMIT, seed=9)
            assert _finite(want) and np.all(raw["moves"] > 0)
            res = ba.snp_ldpred2_auto(sf, df, seed=9, **si.WINDOW_LIMIT)
            same(res, want)
            print("half %d (%s): device seconds per chain %s" % (half, "window" if fits else "general", [r["time"] for r in res]))


# ---- 5. the report columns at their edges ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small65(ba):
    name, A, sub, df = si.small_cases(65)[0]
    assert name == "whole" and sub is None
    with ba.as_SFBM(A) as sf:
        yield A, sf, df


@pytest.mark.parametrize("kw, columns", [(dict(burn_in=0, num_iter=10, report_step=4), 2),
                                         (dict(burn_in=5, num_iter=10, report_step=1), 10),
                                         (dict(burn_in=5, num_iter=10, report_step=10), 1),
                                         (dict(burn_in=5, num_iter=10, report_step=15), 0),
                                         (dict(burn_in=0, num_iter=1, report_step=1), 1)],
                         ids=["no_burn_in", "every_sweep", "last_sweep_only", "no_column", "one_sweep"])
def test_report_edges(ba, small65, kw, columns, monkeypatch):
    A, sf, df = small65
    kw = dict(vec_p_init=si.AUTO_SMALL["vec_p_init"], h2_init=si.AUTO_SMALL["h2_init"], **kw)
    want, raw = _expected(ba, sf, A, df, None, kw)
    assert _finite(want) and np.all(raw["moves"] > 0)
    win, gen = _both_paths(ba, sf, df, None, kw, monkeypatch)
    assert equal_lists(win, gen)
    for res in (win, gen):
        same(res, want)
        for g, r in enumerate(res):
            assert r["sample_beta"].shape == (65, columns)
            assert r["path_p_est"].shape == (kw["burn_in"] + kw["num_iter"],)
            # column c is curr_beta after sweep burn_in + (c + 1) report_step - 1: the causal set of that sweep
            sweeps = kw["burn_in"] + (np.arange(columns) + 1) * kw["report_step"] - 1
            assert np.array_equal(np.count_nonzero(r["sample_beta"], axis=0), raw["path_nb"][sweeps, g])


def test_report_columns_of_a_chain_that_stops(ba, monkeypatch):
    """report_step = 1 on the matrix that is not positive definite: every chain stops within a few sweeps, some after
    having reported.  The columns reported before the stop stay, the others keep the zeros they started with, and the
    last sweep, a report sweep, is never run."""
    A, df = si.diverging_case()
    kw = dict(vec_p_init=P4, h2_init=0.3, burn_in=0, num_iter=10, report_step=1)
    with ba.as_SFBM(A) as sf:
        want, raw = _expected(ba, sf, A, df, None, kw, seed=1)
        stopped = (raw["path_nb"] >= 0).sum(axis=0)                          # sweeps each chain completed
        reported = [np.any(w["sample_beta"] != 0, axis=0) for w in want]
        print("sweeps completed %s, non-zero report columns %s" % (stopped, [int(c.sum()) for c in reported]))
        assert np.all(stopped < 10) and np.any(stopped > 0)                  # checked on the host, before the device runs
        assert any(c.any() for c in reported)
        win, gen = _both_paths(ba, sf, df, None, kw, monkeypatch, seed=1)
        assert equal_lists(win, gen)
        for res in (win, gen):
            same(res, want)
            for g, r in enumerate(res):
                assert r["sample_beta"].shape == (A.shape[0], 10)
                assert np.all(r["sample_beta"][:, stopped[g]:] == 0)
                assert np.array_equal(np.count_nonzero(r["sample_beta"][:, :stopped[g]], axis=0), raw["path_nb"][:stopped[g], g])
                assert np.isnan(r["beta_est"]).all() and np.isnan(r["path_h2_est"][stopped[g]:]).all()
                assert np.isfinite(r["path_h2_est"][:stopped[g]]).all()


# ---- 6. repeated indices --------------------------------------------------------------------------------------------------------------

def test_repeated_indices(ba):
    """the mirror and the library both refuse a repeated ind_corr before any output buffer is written"""
    from bigsnpr_amd import _lib
    from bigsnpr_amd._lib import f64p, i64p, ptr, u64p
    A = si.small_with_empty_columns()
    ind = si.repeated_subset()
    m = ind.size
    df = si.small_df(m, 700)
    with ba.as_SFBM(A) as sf:
        with pytest.raises(ValueError, match="'ind.corr' should not have repeated indices."):
            ba.snp_ldpred2_auto(sf, df, 0.3, vec_p_init=si.AUTO_SMALL["vec_p_init"], ind_corr=ind)
        G, burn_in, num_iter, step = 3, 5, 10, 4
        x, n_vec, log_var = np.random.default_rng(8).normal(size=m), np.full(m, 1500.0), np.zeros(m)
        p_init, stream = np.array([1.0, 0.1, 0.01]), np.arange(G, dtype=np.uint64)
        est = [np.full(m * G, 7.0) for _ in range(3)]
        smp = np.full(m * (num_iter // step) * G, 7.0)
        path = [np.full((burn_in + num_iter) * G, 7.0) for _ in range(3)]
        secs = np.full(G, 7.0)
        rc = _lib.load().bsn_ldpred2_auto(sf.handle, ptr(x, f64p), ptr(n_vec, f64p), ptr(log_var, f64p), m, ptr(ind, i64p),
                                          ptr(p_init, f64p), ptr(stream, u64p), G, 0.3, burn_in, num_iter, step, 0, 1.0, 1, 1e-5,
                                          1.0, -0.5, 1.5, 1.0, 1, ptr(est[0], f64p), ptr(est[1], f64p), ptr(est[2], f64p),
                                          ptr(smp, f64p), ptr(path[0], f64p), ptr(path[1], f64p), ptr(path[2], f64p),
                                          ptr(secs, f64p))
        with pytest.raises(ba.BsnError, match="'ind_sub' has [0-9]+ more than once."):
            _lib.check(rc)
        for buf in est + [smp] + path + [secs]:
            assert np.all(buf == 7.0)
        # the handle works on
        sub = si.small_subsets(65)[0]
        dsub = si.small_df(65, 565, sub)
        same(ba.snp_ldpred2_auto(sf, dsub, ind_corr=sub, seed=si.AUTO_SEED, **si.AUTO_SMALL),
             _expected(ba, sf, A, dsub, sub, si.AUTO_SMALL)[0])
