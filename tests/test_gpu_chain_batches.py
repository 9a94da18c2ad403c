"""The batch loop `for (g0 = 0; g0 < G; g0 += batch)` of the three chain drivers of bigsnpr_amd/csrc/sparse_ld.hip
(bsn_lassosum2, run_gibbs, run_auto).  `batch` is what the free device memory holds, which on a large card is always
the whole call; BSN_CHAIN_BATCH=<n> caps it, so that here the loop goes round again: the chain of a workgroup is
order[g0 + blockIdx.x], the state buffers are reused behind a memset that covers the batch only, and the last batch
is shorter than the others.

Every capped call must equal the uncapped call and the CPU statement (tests/native) bit for bit: a chain's result
depends on its own parameters, the seed and its stream id alone.  The chains have unequal p in an order that is not
the drivers' visiting order (large p first) and stream ids that are not their positions, so a chain that picked up a
neighbour's parameters, stream or state would not pass.  tests/test_sfbm_inputs_cpu.py proves without a GPU that every
chain and grid point moves on these inputs."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import auto_statement  # noqa: E402
import lassosum2_ref  # noqa: E402
import ldpred2_ref  # noqa: E402
import sfbm_inputs as si  # noqa: E402
from auto_statement import equal_lists, same  # noqa: E402

SEED = 77
CASES = ("whole", "ascending", "shuffled")


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def resident(ba):
    cases = si.batch_cases()
    assert tuple(c[0] for c in cases) == CASES
    with ba.as_SFBM(cases[0][1]) as sf:
        yield sf, {name: (A, sub, df) for name, A, sub, df in cases}


def _times_ok(t):
    t = np.asarray(t, dtype=np.float64)
    return bool(np.all(np.isfinite(t)) and np.all(t > 0))


@pytest.mark.parametrize("case", CASES)
def test_lassosum2_in_batches(ba, resident, case, monkeypatch):
    sf, cases = resident
    A, sub, df = cases[case]
    beta, iters, spars, moves = si.lassosum2_statement(lassosum2_ref, A, df, sub=sub, **si.SMALL_LASSO)
    assert beta.shape[1] == 8 and np.all(moves > 0)
    whole = ba.snp_lassosum2(sf, df, ind_corr=sub, **si.SMALL_LASSO)
    assert np.array_equal(np.asarray(whole), beta, equal_nan=True) and np.array_equal(whole.grid_param["num_iter"], iters)
    for cap in si.BATCH_CAPS_LASSO:
        monkeypatch.setenv("BSN_CHAIN_BATCH", str(cap))
        res = ba.snp_lassosum2(sf, df, ind_corr=sub, **si.SMALL_LASSO)
        monkeypatch.delenv("BSN_CHAIN_BATCH")
        assert np.array_equal(np.asarray(res), np.asarray(whole), equal_nan=True), cap
        assert np.array_equal(np.asarray(res), beta, equal_nan=True), cap
        assert np.array_equal(res.grid_param["num_iter"], iters), cap
        assert np.array_equal(res.grid_param["sparsity"], spars, equal_nan=True), cap
        assert _times_ok(res.grid_param["time"]), (cap, res.grid_param["time"])


@pytest.mark.parametrize("case", CASES)
def test_gibbs_in_batches(ba, resident, case, monkeypatch):
    sf, cases = resident
    A, sub, df = cases[case]
    gp = si.BATCH_CHAINS
    kw = {"burn_in": si.SMALL_BURN_IN, "num_iter": si.SMALL_NUM_ITER}
    want, moves = si.gibbs_statement(ldpred2_ref, A, df, gp, SEED, sub=sub, **kw)
    assert want.shape[1] == 5 and np.all(moves > 0) and np.isfinite(want).all()
    for no_window in (False, True):
        if no_window:
            monkeypatch.setenv("BSN_GIBBS_NO_WINDOW", "1")
        whole = ba.snp_ldpred2_grid(sf, df, gp, ind_corr=sub, seed=SEED, **kw)
        assert np.array_equal(np.asarray(whole), want, equal_nan=True), no_window
        for cap in si.BATCH_CAPS:
            monkeypatch.setenv("BSN_CHAIN_BATCH", str(cap))
            res = ba.snp_ldpred2_grid(sf, df, gp, ind_corr=sub, seed=SEED, **kw)
            monkeypatch.delenv("BSN_CHAIN_BATCH")
            assert np.array_equal(np.asarray(res), np.asarray(whole), equal_nan=True), (no_window, cap)
            assert np.array_equal(np.asarray(res), want, equal_nan=True), (no_window, cap)
            assert np.array_equal(res.grid_param["stream"], gp["stream"]) and _times_ok(res.grid_param["time"]), (no_window, cap)
        if no_window:
            monkeypatch.delenv("BSN_GIBBS_NO_WINDOW")


@pytest.mark.parametrize("case", CASES)
def test_auto_in_batches(ba, resident, case, monkeypatch):
    sf, cases = resident
    A, sub, df = cases[case]
    kw = si.BATCH_AUTO
    mean_ld = float(np.mean(ba.ld_scores_sfbm(sf, sub)))
    want, raw = auto_statement.expected(si.full_of(A), df, mean_ld, seed=SEED, sub=sub, **kw)
    assert len(want) == 5 and np.all(raw["moves"] > 0)
    for no_window in (False, True):
        if no_window:
            monkeypatch.setenv("BSN_GIBBS_NO_WINDOW", "1")
        whole = ba.snp_ldpred2_auto(sf, df, ind_corr=sub, seed=SEED, **kw)
        same(whole, want)
        for cap in si.BATCH_CAPS:
            monkeypatch.setenv("BSN_CHAIN_BATCH", str(cap))
            res = ba.snp_ldpred2_auto(sf, df, ind_corr=sub, seed=SEED, **kw)
            monkeypatch.delenv("BSN_CHAIN_BATCH")
            assert equal_lists(res, whole), (no_window, cap)
            same(res, want)
            assert [r["stream"] for r in res] == [int(s) for s in kw["stream"]]
            assert _times_ok([r["time"] for r in res]), (no_window, cap)
        if no_window:
            monkeypatch.delenv("BSN_GIBBS_NO_WINDOW")


def test_a_cap_below_one_or_above_the_call_changes_nothing(ba, resident, monkeypatch):
    sf, cases = resident
    A, sub, df = cases["ascending"]
    kw = si.BATCH_AUTO
    whole = ba.snp_ldpred2_auto(sf, df, ind_corr=sub, seed=SEED, **kw)
    for cap in ("0", "-3", "", "100"):
        monkeypatch.setenv("BSN_CHAIN_BATCH", cap)
        res = ba.snp_ldpred2_auto(sf, df, ind_corr=sub, seed=SEED, **kw)
        monkeypatch.delenv("BSN_CHAIN_BATCH")
        assert equal_lists(res, whole), cap
