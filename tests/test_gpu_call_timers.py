"""The device times that the one-shot entries report about their last call (bsn_impute_last_ms, bsn_popstat_last_ms,
bsn_project_last_ms, bsn_sfbm_last_ms, bsn_plr_last_stats): all of them come from one shared set of HIP events
(EventMarks, bigsnpr_amd/csrc/bsn_internal.hpp), and only the probes under tools/ read them otherwise.

Each case makes one small call and reads the entry: every slot is finite and >= 0, the slot of a phase that ran is > 0,
the slot of a phase that did not run is exactly 0 (also where an earlier call of the process had left a time there).
There is no bound on any time."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import plr_inputs  # noqa: E402
import sfbm_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

N, M = 130, 70


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def image(ba):
    """130 x 70 synthetic calls, 3 % of them missing"""
    gb = ba.bed.synthetic(N, M, seed=7, npop=3, na16=1966)
    assert ba.bed_counts(gb)[3].sum() > 0
    yield gb
    gb.close()


def _slots(ms, ran, idle):
    ms = np.asarray(ms, dtype=np.float64)
    print("ms", ms)
    assert np.isfinite(ms).all() and (ms >= 0).all(), ms
    assert all(ms[k] > 0 for k in ran), (ms, ran)
    assert all(ms[k] == 0 for k in idle), (ms, idle)


def test_impute_without_fbm_bytes(ba, image):
    res = ba.snp_fastImputeSimple(image, "mode")
    ms = (C.c_double * 3)()
    ba._lib.check(ba.load().bsn_impute_last_ms(ms))
    _slots(list(ms), ran=(0,), idle=(2,))
    assert res.shape == (N, M)


def test_fst_from_counts_then_from_host_frequencies(ba, image):
    from bigsnpr_amd.popstat import popstat_last_ms
    group = np.arange(N) % 3
    ba.bed_fst(image, group, n_groups=3)
    _slots(popstat_last_ms(), ran=(0, 1, 2, 3), idle=())
    # the same statistic from host frequencies: no counting pass, and the times of the call above are cleared
    ba.snp_fst(ba.bed_MAF_by_group(image, group, n_groups=3))
    _slots(popstat_last_ms(), ran=(3,), idle=(0, 1, 2))


def test_oadp_projection_alone(ba):
    rng = np.random.default_rng(3)
    n, K = 40, 3
    d = np.array([9.0, 5.0, 2.0])
    XV = rng.normal(size=(n, K)) * d
    X_norm = (XV ** 2).sum(axis=1) + rng.uniform(0.1, 1.0, n)
    out = ba.pca_OADP_proj_device(XV, X_norm, d)
    assert np.isfinite(out).all()
    _slots(ba.prs.project_last_ms(), ran=(1,), idle=(0,))


def test_project_pca_fused(ba, image):
    rng = np.random.default_rng(4)
    K = 3
    stats = ba.bed_colstats(image)
    center = stats["sumX"] / stats["nb_nona_col"]
    scale = np.sqrt(np.maximum(stats["denoX"], 1.0))
    V = rng.normal(size=(M, K))
    ba.project_pca(image, None, np.arange(M), center, scale, V, np.array([9.0, 5.0, 2.0]))
    _slots(ba.prs.project_last_ms(), ran=(0, 1), idle=())


def test_sparse_product(ba):
    A = sfbm_inputs.as_full(sfbm_inputs.banded_corr(60, 6, seed=5))
    x = np.random.default_rng(6).normal(size=60)
    with ba.as_SFBM(A) as sf:
        y = ba.sp_prodVec(sf, x)
        _slots([sf.last_ms()], ran=(0,), idle=())
    assert np.isfinite(y).all()


def test_penalised_regression_stats_add_up(ba):
    """[0] sweeps, [1] scans, [2] turns of the host loop, [4] start, [5] their total"""
    case = plr_inputs.case_small(*plr_inputs.SMALL_SHAPES[0], dense=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ba.big_spLinReg(ba.FBM_code256(case["codes"]), case["ys"]["linear"], **plr_inputs.dev_kw(case))
    out = (C.c_double * 6)()
    ba._lib.check(ba.load().bsn_plr_last_stats(out))
    st = np.array(list(out))
    print("plr stats", st)
    assert np.isfinite(st).all() and (st >= 0).all()
    assert abs(st[5] - (st[4] + st[0] + st[1])) <= 1e-12 * st[5]
    assert st[2] >= 1
