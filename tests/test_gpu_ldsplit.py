"""snp_ldsplit on the device against the CPU statement (tests/native/ldsplit_ref.cpp): C (+Inf included), best_ind, cost,
cost2, perc_kept, all_last and levels_run with np.array_equal — integers and float bits, no tolerance anywhere.  The inputs
are those of tests/helpers/ldsplit_inputs.py (tests/test_ldsplit_cpu.py proves what each contains); the shapes follow the
tile constants of ldsplit.hip."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ldsplit_ref as ref  # noqa: E402

sparse = pytest.importorskip("scipy.sparse")
import ldsplit_inputs as inputs  # noqa: E402

INF = float("inf")
K = inputs.kernel_constants()
TILE, SPLIT = K["kRowTile"], K["kSplit"]
EQUAL = ("C", "best_ind", "cost", "cost2", "perc_kept", "ok", "all_last", "levels_run")


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def _kw(kw, **over):
    out = dict(kw)
    out.update(over)
    return out


def _cases():
    """name -> (matrix, arguments, handed over as upper triangle?)"""
    cases = {}
    for n, name in enumerate(inputs.NAMES):
        A, kw = inputs.named(name)
        cases[name] = (A, kw, n % 2 == 0)
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def statement():
    done = {}

    def get(name):
        if name not in done:
            A, kw, _ = CASES[name]
            p, i, x = ref.csc(A)
            done[name] = ref.split(p, i, x, A.shape[0], **kw)
        return done[name]
    return get


def _device(ba, A, kw, upper):
    from bigsnpr_amd.ldsplit import ldsplit_one
    with ba.as_SFBM(sparse.csc_matrix(sparse.triu(A)) if upper else A, upper=upper) as sf:
        return ldsplit_one(sf, **kw)


def _same(got, exp):
    for key in EQUAL:
        assert np.array_equal(got[key], exp[key]), key


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_statement(ba, statement, name):
    A, kw, upper = CASES[name]
    W = kw["max_size"] - kw["min_size"] + 1
    if name in ("ties", "max_r2", "window"):
        assert W > 4 * SPLIT and A.shape[0] % TILE == {"ties": 1, "max_r2": TILE - 1, "window": 0}[name]
    exp = statement(name)
    if name != "level_0_only":
        assert exp["ok"].any()
    _same(_device(ba, A, kw, upper), exp)


def test_early_stop_leaves_the_rest_untouched(ba, statement):
    A, kw, upper = CASES["early_stop"]
    got = _device(ba, A, kw, upper)
    lv = got["levels_run"]
    assert 1 < lv < kw["max_K"] and lv == statement("early_stop")["levels_run"]
    assert np.all(np.isinf(got["C"][:, lv:])) and np.all(got["best_ind"][:, lv:] == -1)


def test_costs_are_the_r2_outside_the_device_s_own_blocks(ba):
    """independent of the statement: dyadic entries, so the float of E and every sum are exact"""
    A, kw, upper = CASES["moderate"]
    got = _device(ba, A, kw, upper)
    assert got["ok"].sum() > 10
    for kk in np.nonzero(got["ok"])[0]:
        last = got["all_last"][kk, :kk + 1].astype(np.int64) - 1
        size = np.diff(np.concatenate([[-1], last]))
        assert last[-1] == A.shape[0] - 1 and np.all((size >= kw["min_size"]) & (size <= kw["max_size"]))
        assert got["cost"][kk] == inputs.outside_cost(A, last, kw["thr_r2"])[0] and got["cost2"][kk] == np.sum(size ** 2)


def test_several_max_size_through_snp_ldsplit(ba):
    A, _ = inputs.named("ties")
    args = dict(max_K=40, max_r2=1.0, max_cost=INF)
    exp = ref.snp_ldsplit(A, 0.0, 4, [30, 12, 20], **args)
    for corr in (A, sparse.csc_matrix(sparse.triu(A))):
        got = ba.snp_ldsplit(corr, 0.0, 4, [30, 12, 20], **args)
        assert sorted(got) == sorted(exp) and len(set(exp["max_size"].tolist())) > 1
        for col in ("max_size", "n_block", "cost", "cost2", "perc_kept"):
            assert np.array_equal(got[col], exp[col]), col
        for col in ("all_last", "all_size"):
            assert len(got[col]) == len(exp[col]) and all(np.array_equal(a, b) for a, b in zip(got[col], exp[col])), col
    # the default max_cost (m / 200) leaves nothing on this matrix
    assert ba.snp_ldsplit(A, 0.0, 4, 30, max_K=5) is None and ref.snp_ldsplit(A, 0.0, 4, 30, max_K=5) is None


def test_refusals_leave_the_handle_usable(ba, statement):
    from bigsnpr_amd.ldsplit import ldsplit_one
    A, kw, _ = CASES["thr_r2"]
    m = A.shape[0]
    with ba.as_SFBM(A, upper=False) as sf:
        with pytest.raises(ba.BsnError, match="'max_size' .* must be at most ncol"):
            ldsplit_one(sf, **_kw(kw, max_size=m + 1))
        with pytest.raises(ba.BsnError, match="'pos_scaled' must be ascending"):
            pos = np.arange(m, dtype=np.float64)
            pos[[10, 11]] = pos[[11, 10]]
            ldsplit_one(sf, **_kw(kw, pos_scaled=pos))
        with pytest.raises(ba.BsnError, match="'min_size' must be at least 1"):
            ldsplit_one(sf, **_kw(kw, min_size=0))
        _same(ldsplit_one(sf, **kw), statement("thr_r2"))
    B = sparse.lil_matrix(A)
    B[33, 33] = 0
    B = sparse.csc_matrix(B)
    B.eliminate_zeros()
    with ba.as_SFBM(B, upper=False) as sf:
        with pytest.raises(ba.BsnError, match="must store its diagonal: column 33 has none"):
            ldsplit_one(sf, **kw)
        y = ba.sp_prodVec(sf, np.ones(m))
        assert np.allclose(y, B @ np.ones(m))
