"""big_spLinReg / big_spLogReg on the device past the first turn of every loop of bigsnpr_amd/csrc/plr.hip.

The inputs are tests/helpers/plr_inputs.py's seeded cases; tests/test_plr_inputs_cpu.py proves on the CPU statement, in both
summation orders, that each case reaches the loop turn or branch it is named for.  Every case is held to the statement
(tests/native/plr_ref.cpp) on the decoded matrix by tests/helpers/plr_check.py, the rule of tests/test_gpu_plr.py:
discrete outputs equal exactly, continuous ones within 1000 x the spread of the statement's two orders on that input."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import plr_inputs as inp  # noqa: E402
import dosage_inputs as dos  # noqa: E402
from plr_check import _fit, _raw, _same  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = inp.FAMILIES


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def _on_device(ba, case):
    """what the device is given: the 2-bit image of the calls, or the dense matrix in its own type"""
    if case["codes"] is None:
        return case["dense"]
    G = ba.FBM_code256(case["codes"])
    assert G.bits == 2
    return G


def _host_turns(ba):
    """the turns of the last call's host loop (bsn_plr_last_stats)"""
    out = (C.c_double * 6)()
    ba.load().bsn_plr_last_stats(out)
    return int(out[2])


def _run(ba, case, family, X=None, **dev_over):
    """one call on the device, checked against the statement; returns (the model, the statement's forward outputs).
    The chains run in lockstep from the first turn and a chain is live for as many turns as the statement calls its sweep
    after l = 0, so the host loop takes exactly max(turns) turns: one more discrete output that has to be equal"""
    t0 = time.perf_counter()
    mod = _fit(ba, family, _on_device(ba, case) if X is None else X, case["ys"][family], **inp.dev_kw(case, **dev_over))
    dt, turns = time.perf_counter() - t0, _host_turns(ba)
    where = "%s, %s" % (case["name"], family)
    f = _same(mod, case["X"], case["ys"][family], case["fold"], case["K"], where, **inp.ref_kw(case, family))
    print("%s: %.3f s on the device, %d turns of the host loop (statement: %d)" % (where, dt, turns, f["turns"].max()))
    assert turns == f["turns"].max(), (where, turns, f["turns"])
    return mod, f


@pytest.mark.parametrize("family", FAMILIES)
def test_a_active_set_across_1024(ba, family):
    """compact's second turn with `base` carried over, the count and copy loops of k_plr_commit and the sweep's walk of
    the list past 1024 entries: every chain has fewer than 1024 non-zeros at one lambda and more at a later one"""
    mod, f = _run(ba, inp.case_active_set_across_1024(), family)
    nb = f["nb_active"]
    assert (nb[1] < 1024).all() and (nb[11] > 1024).all() and set(f["status"]) == {4}


@pytest.mark.parametrize("family", FAMILIES)
def test_b_lambda_max_from_a_column_past_1024(ba, family):
    """k_plr_lmax's stride loop: column 1090 decides lambda_max in every chain; the grid itself is compared"""
    case = inp.case_lambda_max_past_1024()
    mod, f = _run(ba, case, family)
    for c in range(2):
        lam = mod[0][c]["lambda"]
        assert inp.lambda_max_below(case, family, c, 1024) < 0.9 * lam[0]
        np.testing.assert_allclose(lam, f["lambda"][:lam.size, c], rtol=1e-12, atol=0)
        assert f["beta"][1090, c] != 0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("family", FAMILIES)
def test_c_chain_blocks(ba, family, order):
    """k_plr_scan over twelve chains: order 0 leaves block 0 (chains 0 - 7) all dead while block 1 runs (`continue`, then
    a live block); order 1 leaves block 1 all dead and block 0 half dead (`live[u]` mixed inside a block)"""
    mod, f = _run(ba, inp.case_chain_blocks(order), family)
    t = f["turns"]
    assert t[0:8].max() < t[8:12].min() if order == 0 else t[4:12].max() < t[0:4].min(), t


@pytest.mark.parametrize("max_iter", [1, 3])
@pytest.mark.parametrize("family", FAMILIES)
def test_d_max_iter(ba, family, max_iter):
    """a sweep that returns at the cap and a commit that closes the lambda on `iter_l >= max_iter`"""
    mod, f = _run(ba, inp.case_max_iter(max_iter), family)
    assert (f["iter"][1:] == max_iter).all() and set(f["status"]) == {4}
    assert all((mo["iter"][1:] == max_iter).all() and mo["iter"].size == 10 for mods in mod for mo in mods)


@pytest.mark.parametrize("family", FAMILIES)
def test_e_penalty_factors(ba, family):
    """two unpenalised X columns as the start set (k_plr_init's flags), a penalised covariate entering at j >= m"""
    mod, f = _run(ba, inp.case_penalty_factors(), family)
    assert (f["nb_active"][0] == 2).all() and (f["beta"][40] != 0).any()
    got = _raw(mod)
    assert all((nb[0] == 2) for nb in got["nb_active"]) and (got["beta"][[3, 17]] != 0).all() and (got["beta"][40] != 0).any()


def test_f_model_saturated(ba):
    """kSaturated through book() in k_plr_commit"""
    mod, f = _run(ba, inp.case_saturated(), "logistic")
    assert set(f["status"]) == {3}
    assert [mo["message"] for mo in mod[0]] == ["Model saturated"] * 3


@pytest.mark.parametrize("dense", [False, True], ids=["2bit", "float64"])
@pytest.mark.parametrize("family", FAMILIES)
def test_g_constant_columns(ba, family, dense):
    """k_plr_stats<0>: n0 == nt, v[0] == nt, v[1] == nt, on every fold and on one fold only; k_plr_stats<2>: lo == hi at
    0.1 and at 1 / 3 (whose mean in the kernel's own tree is not 1 / 3: without the line the column gets a scale of
    1e16), on every fold and on one fold only"""
    case = inp.case_constant_columns(dense)
    mod, f = _run(ba, case, family)
    got = _raw(mod)["beta"]
    z = np.zeros(got.shape, dtype=bool)
    for j, c in (inp.G_ZERO_DENSE if dense else inp.G_ZERO_2BIT):
        z[j, c] = True
    assert (got[z] == 0).all() and (got[~z] != 0).any() and np.isfinite(got).all()


@pytest.mark.parametrize("dense", [False, True], ids=["2bit", "float64"])
def test_h_everything_monomorphic(ba, dense):
    """lambda_max = 0: a grid of zeros, nothing enters, "No more improvement" after four lambdas"""
    mod, f = _run(ba, inp.case_monomorphic(dense), "linear")
    assert set(f["status"]) == {1} and set(f["n_done"]) == {4}
    for mo in mod[0]:
        assert mo["lambda"].size == 4 and (mo["lambda"] == 0).all() and (mo["beta"] == 0).all()
        assert mo["message"] == "No more improvement"


@pytest.mark.parametrize("dense", [False, True], ids=["2bit", "float32"])
@pytest.mark.parametrize("n,m", inp.SMALL_SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_i_small_shapes(ba, family, n, m, dense):
    """n below one wave, at one wave and one past it; a single column: most of the 1024 (256) threads hold no row"""
    case = inp.case_small(n, m, dense)
    if dense:
        assert case["dense"].dtype == np.float32
    _run(ba, case, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_j_byte_image_through_a_selection(ba, family):
    """KIND 1 behind image_gather (an unsorted row list, every other column) with two unpenalised covariates"""
    k, rows, cols, case = inp.case_byte_selection()
    D = ba.FBM_code256(dos.dosage_bytes(k), code=ba.CODE_DOSAGE)
    assert D.bits == 8
    mod, f = _run(ba, case, family, X=D, ind_train=rows, ind_col=cols)
    assert (f["beta"][30:] != 0).all() and mod.n_covar == 2 and np.array_equal(mod.ind_col, cols)


def _dense_abi(ba, A, ld, case, family):
    """bsn_dense_sp_reg called directly on the buffer A (ld rows per column); the raw outputs"""
    from bigsnpr_amd import _lib
    n, m = case["X"].shape
    K, kw = case["K"], case["kw"]
    y = np.ascontiguousarray(case["ys"][family], dtype=np.float64)
    pf = np.ones(m)
    alphas = np.asarray(kw["alphas"], dtype=np.float64)
    NL, Cn = kw["nlambda"], K * alphas.size
    opt = _lib.PlrOptions(int(family == "logistic"), NL, kw["nlam_min"], kw["n_abort"], 50000, kw["max_iter"], kw["eps"],
                          kw["lambda_min_ratio"])
    out = dict(intercept=np.empty(Cn), beta=np.empty((m, Cn), order="F"))
    for name in ("lambda", "loss", "loss_val"):
        out[name] = np.empty((NL, Cn), order="F")
    for name in ("iter", "nb_active"):
        out[name] = np.empty((NL, Cn), dtype=np.int32, order="F")
    for name in ("n_done", "best", "status"):
        out[name] = np.empty(Cn, dtype=np.int32)
    f64p, i32p, ptr = _lib.f64p, _lib.i32p, _lib.ptr
    _lib.check(_lib.load().bsn_dense_sp_reg(
        A.ctypes.data_as(C.c_void_p), 4 if A.dtype == np.float32 else 7, ld, n, m, ptr(y, f64p), None, 0, ptr(pf, f64p),
        ptr(case["fold"], i32p), K, ptr(alphas, f64p), alphas.size, C.byref(opt), ptr(out["intercept"], f64p),
        ptr(out["beta"], f64p), ptr(out["lambda"], f64p), ptr(out["loss"], f64p), ptr(out["loss_val"], f64p),
        ptr(out["iter"], i32p), ptr(out["nb_active"], i32p), ptr(out["n_done"], i32p), ptr(out["best"], i32p),
        ptr(out["status"], i32p)))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["type4", "type7"])
@pytest.mark.parametrize("family", FAMILIES)
def test_k_leading_dimension_at_the_abi(ba, family, dtype):
    """bsn_dense_sp_reg with ld = n + 3 and NaN in the three pad rows of every column: every output has the bits of the
    same call on the contiguous copy (ld = n), NaN of the lambdas not reached included"""
    case = inp.case_max_iter(3)
    n, m = case["X"].shape
    padded = np.full((n + 3, m), np.nan, dtype=dtype, order="F")
    padded[:n] = case["X"]
    tight = np.asfortranarray(case["X"].astype(dtype))
    assert np.isnan(padded[n:]).all() and np.array_equal(padded[:n], tight)
    a = _dense_abi(ba, padded, n + 3, case, family)
    b = _dense_abi(ba, tight, n, case, family)
    for name in a:
        assert a[name].tobytes(order="A") == b[name].tobytes(order="A"), (family, name)
        assert np.array_equal(a[name], b[name]), (family, name)      # (every lambda is reached: no NaN left)
    assert np.isfinite(a["beta"]).all() and (a["beta"] != 0).any() and set(a["n_done"]) == {10}
