"""snp_ancestry_summary / bed_ancestry on the device (bigsnpr_amd/csrc/ancestry.hip) against the CPU statement compiled from
the same qp_step.hpp (tests/native/ancestry_ref.cpp) and against the program's definition (tests/ancestry_cases.py).  The
device and the statement sum in different orders (a butterfly over the group against a plain loop): objectives are compared,
not bits.  tests/test_ancestry_cpu.py holds the statement to the definition."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ancestry_cases as cases  # noqa: E402
import ancestry_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


per_workgroup, same_minimiser = cases.per_workgroup, cases.same_minimiser


# ---- G1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 8, 9, 16, 17, 19, 32, 33, cases.CAP])
def test_qp_simplex_shapes(ba, K):
    pw = per_workgroup(K)
    counts = sorted({b for b in (1, pw - 1, pw, pw + 1, 4 * pw + 3) if b >= 1})
    for B in counts:
        D, d = cases.problem_batch(K, B, 1000 * K + B)
        well = np.linalg.cond(D) <= 1e4
        for s1 in (True, False):
            got, want = ba.qp_simplex(D, d, s1), ref.qp_simplex(D, d, s1)
            assert got["n_failed"] == 0 and want["n_failed"] == 0 and (got["steps"] >= 0).all()
            assert got["w"].shape == (B, K) and got["w"].flags.f_contiguous
            for b in range(B):
                same_minimiser(D, d[:, b], got["w"][b], want["w"][b], s1, (K, B, s1, b))
            if well:
                assert np.abs(got["w"] - want["w"]).max() <= 1e-10, (K, B, s1)


@pytest.mark.parametrize("K", [9, 19, 33])
def test_qp_simplex_ill_conditioned(ba, K):
    D, d = cases.problem_batch(K, 2 * per_workgroup(K) + 1, 77 + K, ba.nearPD)
    assert np.linalg.cond(D) > 1e7
    for s1 in (True, False):
        got, want = ba.qp_simplex(D, d, s1), ref.qp_simplex(D, d, s1)
        assert got["n_failed"] == 0
        for b in range(d.shape[1]):
            same_minimiser(D, d[:, b], got["w"][b], want["w"][b], s1, (K, s1, b))


def test_qp_simplex_case_list(ba):
    for name, D, d, s1, w_known in cases.qp_cases(ba.nearPD):
        got, want = ba.qp_simplex(D, d, s1), ref.qp_simplex(D, d, s1)
        assert got["n_failed"] == 0, name
        same_minimiser(D, d, got["w"][0], want["w"][0], s1, name)
        if w_known is not None:
            assert np.abs(got["w"][0] - w_known).max() <= 1e-9, name
    D = np.eye(3) + 0.1
    d = np.array([[0.3, np.nan, 0.1], [0.2, 0.5, np.inf], [0.1, 0.2, 0.3]]).T
    r = ba.qp_simplex(D, d)
    assert np.isnan(r["w"][:2]).all() and list(r["steps"][:2]) == [-1, -1] and r["n_failed"] == 0
    cases.check_solution(D, d[:, 2], r["w"][2], True)


# ---- G2 ----------------------------------------------------------------------------------------------------------------
def test_refusals(ba):
    cap = ba.load().bsn_qp_max_k()
    assert cap == cases.CAP == ref.max_k()
    with pytest.raises(ba.BsnError, match="at least one reference group"):
        ba.qp_simplex(np.zeros((0, 0)), np.zeros((0, 1)))
    with pytest.raises(ba.BsnError, match="more than 60 reference groups"):
        ba.qp_simplex(np.eye(cap + 1), np.zeros(cap + 1))
    with pytest.raises(ba.BsnError, match="not positive definite"):
        ba.qp_simplex(np.array([[1.0, 2.0], [2.0, 1.0]]), np.zeros(2))
    rng = np.random.default_rng(1)
    M = 50
    with pytest.raises(ba.BsnError, match="more than 64 columns of 'projection'"):
        ba.ancestry_moments(rng.normal(size=(M, 65)), rng.uniform(size=(M, 3)))
    with pytest.raises(ba.BsnError, match="more than 60 reference groups"):
        ba.ancestry_moments(rng.normal(size=(M, 2)), rng.uniform(size=(M, cap + 1)))
    # a Dmat without a Cholesky factor, through the raw entry: refused, and the results are not touched
    P, X0, F = (np.asfortranarray(a) for a in (rng.normal(size=(M, 2)), rng.uniform(size=(M, 3)), rng.uniform(size=(M, 1))))
    bad = np.asfortranarray(-np.eye(3))
    w = np.full((1, 3), 7.0, order="F")
    ce, cp, steps, corr = np.zeros((1, 3), order="F"), np.zeros(1), np.zeros(1, dtype=np.int32), np.ones(2)
    p = lambda a: a.ctypes.data_as(f64p)   # noqa: E731
    rc = ba.load().bsn_ancestry_summary(p(F), M, 1, p(X0), M, p(P), M, p(corr), M, 2, 3, p(bad), 1, 0, p(w), p(ce), p(cp),
                                        steps.ctypes.data_as(i32p))
    assert rc != 0 and (w == 7.0).all()
    with pytest.raises(ba.BsnError, match="leading dimension"):
        ba._lib.check(ba.load().bsn_ancestry_moments(p(P), M - 1, p(X0), M, None, M, M, 2, 3, 0, 0, *([None] * 7)))
    # a dosage image has no 2-bit genotype
    dos = ba.FBM_code256(np.zeros((8, 16), dtype=np.uint8), code=ba.CODE_DOSAGE)
    with pytest.raises(ba.BsnError, match="bed_ancestry is not available for this handle"):
        ba.bed_ancestry(dos, rng.uniform(size=(16, 3)), rng.normal(size=(16, 2)), np.ones(2))


# ---- G3 ----------------------------------------------------------------------------------------------------------------
def _moment_bounds(P, X0, F):
    """numpy fp64 and the bound on reordering a sum of M products, M 2^-52 sum |terms|, per entry"""
    M = P.shape[0]
    eps = M * 2.0 ** -52
    aP, aX, aF = np.abs(P), np.abs(X0), np.abs(F)
    return dict(PtX0=(P.T @ X0, eps * (aP.T @ aX)), PtF=(P.T @ F, eps * (aP.T @ aF)), G0=(X0.T @ X0, eps * (aX.T @ aX)),
                X0tF=(X0.T @ F, eps * (aX.T @ aF)), csX0=(X0.sum(0), eps * aX.sum(0)), csF=(F.sum(0), eps * aF.sum(0)),
                sqF=((F * F).sum(0), eps * (F * F).sum(0)))


@pytest.mark.parametrize("M", ["1", "slab-1", "slab", "slab+1", "2slab+3"])
def test_moments(ba, monkeypatch, M):
    slab = ref.slab_rows()
    M = {"1": 1, "slab-1": slab - 1, "slab": slab, "slab+1": slab + 1, "2slab+3": 2 * slab + 3}[M]
    rng = np.random.default_rng(M)
    Pall, Xall, Fall = rng.normal(size=(M, 17)), rng.uniform(size=(M, 32)), rng.uniform(size=(M, 3))
    for L in (1, 16, 17):
        for K in (1, 19, 32):
            for B in (0, 1, 3):
                P, X0, F = Pall[:, :L], Xall[:, :K], Fall[:, :B]
                want = _moment_bounds(P, X0, F)
                first = None
                for S in (None, 1, 2, 5):
                    if S is None:
                        monkeypatch.delenv("BSN_ANC_SLABS", raising=False)
                    else:
                        monkeypatch.setenv("BSN_ANC_SLABS", str(S))
                    got = ba.ancestry_moments(P, X0, F, ld=M + 5)     # NaN below the rows
                    for k, (ref_v, bound) in want.items():
                        assert got[k].shape == ref_v.shape
                        assert (np.abs(got[k] - ref_v) <= bound).all(), (M, L, K, B, S, k, np.abs(got[k] - ref_v).max())
                    if S is None:
                        first = got
                        again = ba.ancestry_moments(P, X0, F, ld=M + 5)
                        for k in want:
                            assert np.array_equal(again[k], first[k]), (M, L, K, B, k)       # two runs: equal bits


@pytest.mark.parametrize("L,K,B", [(40, 32, 0), (40, 25, 3), (64, 60, 3), (64, 60, 6), (17, 32, 40)])
def test_moments_wide_tables(ba, monkeypatch, L, K, B):
    """more than 64 rows of sums (the kernels with eight rows per thread), and more frequency columns than one launch takes"""
    M = ref.slab_rows() + 77
    rng = np.random.default_rng(L + K + B)
    P, X0, F = rng.normal(size=(M, L)), rng.uniform(size=(M, K)), rng.uniform(size=(M, B))
    want = _moment_bounds(P, X0, F)
    for S in (None, 3):
        if S is None:
            monkeypatch.delenv("BSN_ANC_SLABS", raising=False)
        else:
            monkeypatch.setenv("BSN_ANC_SLABS", str(S))
        got = ba.ancestry_moments(P, X0, F, ld=M + 1)
        for k, (ref_v, bound) in want.items():
            assert (np.abs(got[k] - ref_v) <= bound).all(), (S, k, np.abs(got[k] - ref_v).max())


# ---- G4 ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ex():
    return {L: cases.example_tables(L) for L in (25, 10)}


def _problem(t):
    """(X, D) as the mirror forms them, in numpy"""
    from bigsnpr_amd.ancestry import nearPD
    X = t["P"].T @ t["X0"]
    D, ok = nearPD(X.T @ X)
    assert ok
    return X, D


@pytest.mark.parametrize("L", [25, 10])
def test_summary_end_to_end(ba, ex, L):
    import pandas as pd
    t = ex[L]
    X, D = _problem(t)
    names = ["POP%d" % k for k in range(1, 20)]
    res = ba.snp_ancestry_summary(t["freq"], pd.DataFrame(t["X0"], columns=names), t["P"], t["corr"])
    assert isinstance(res, ba.AncestryProportions) and res.shape == (19,) and res.names == names
    assert res.cor_pred > 1 - 1e-9 and res.steps >= 0 and len(res.ms) == 3
    assert np.array_equal(np.asarray(res), np.round(res.unrounded, 7))
    want_each = [np.corrcoef(t["X0"][:, k], t["freq"])[0, 1] for k in range(19)]
    assert np.abs(res.cor_each - want_each).max() <= 1e-10
    d = X.T @ ((t["P"].T @ t["freq"]) * t["corr"])
    cases.check_solution(D, d, res.unrounded, True)
    if L == 25:
        assert np.abs(res.unrounded - t["wt"]).max() <= 1e-7
        assert np.abs(np.asarray(res) - t["wt"]).max() <= 1e-7

    # M x 3: a second mixture, and a reversed column that comes back NaN (nothing is raised)
    w2 = np.zeros(19)
    w2[[3, 11]] = 0.25, 0.75
    F = np.stack([t["freq"], 1.0 - t["freq"], t["X0"] @ w2], axis=1)
    res = ba.snp_ancestry_summary(F, t["X0"], t["P"], t["corr"])
    assert res.shape == (3, 19) and res.names is None and res.cor_pred.shape == (3,)
    assert np.isnan(res[1]).all() and np.isfinite(res[0]).all() and np.isfinite(res[2]).all()
    assert (res.cor_pred[[0, 2]] > 1 - 1e-9).all()
    for b, wt in ((0, t["wt"]), (2, w2)):
        d = X.T @ ((t["P"].T @ F[:, b]) * t["corr"])
        cases.check_solution(D, d, res.unrounded[b], True)
        if L == 25:
            assert np.abs(res.unrounded[b] - wt).max() <= 1e-7


# ---- G5 ----------------------------------------------------------------------------------------------------------------
def _check_rows(t, X, D, res, G, X0, P):
    """every row of a bed_ancestry result against the definition and np.corrcoef on the decoded rows (no missing value)"""
    n = G.shape[0]
    assert res.shape == (n, X0.shape[1]) and res.cor_pred.shape == (n,) and (res.steps >= 0).all()
    Fr = G.T / 2.0
    dall = X.T @ ((P.T @ Fr) * t["corr"][:, None])
    for i in range(n):
        cases.check_solution(D, dall[:, i], res.unrounded[i], True, i)
    Xc = X0 - X0.mean(0)
    Fc = Fr - Fr.mean(0)
    each = (Xc.T @ Fc) / np.sqrt(np.outer((Xc * Xc).sum(0), (Fc * Fc).sum(0)))
    assert np.abs(res.cor_each - each.T).max() <= 1e-10
    pred = X0 @ res.unrounded.T
    Pc = pred - pred.mean(0)
    cp = (Pc * Fc).sum(0) / np.sqrt((Pc * Pc).sum(0) * (Fc * Fc).sum(0))
    assert np.abs(res.cor_pred - cp).max() <= 1e-10


@pytest.mark.parametrize("L", [25, 10])
def test_bed_ancestry(ba, ex, L):
    t = ex[L]
    X, D = _problem(t)
    gb = ba.bed(os.path.join(GOLDEN, "example.bed"))
    n, m = t["G"].shape
    res = ba.bed_ancestry(gb, t["X0"], t["P"], t["corr"], min_cor=0)
    _check_rows(t, X, D, res, t["G"], t["X0"], t["P"])
    assert len(res.ms) == 3 and (res.ms > 0).all()
    if L == 25:
        share = (np.argmax(res.unrounded, axis=1) == t["own"]).mean()
        print("largest weight on the sample's own label: %.1f %%" % (100 * share))
        assert share >= 0.70
    rows = np.arange(3, n, 7)
    sub = ba.bed_ancestry(gb, t["X0"], t["P"], t["corr"], ind_row=rows, min_cor=0)
    _check_rows(t, X, D, sub, t["G"][rows], t["X0"], t["P"])
    assert np.array_equal(sub.unrounded, res.unrounded[rows])               # a row depends on that row alone
    perm = np.random.default_rng(3).permutation(m)
    pr = ba.bed_ancestry(gb, t["X0"][perm], t["P"][perm], t["corr"], ind_col=perm, min_cor=0)
    _check_rows(t, X, D, pr, t["G"][:, perm], t["X0"][perm], t["P"][perm])
    one = ba.bed_ancestry(gb, t["X0"], t["P"], t["corr"], ind_row=[n - 1], min_cor=0)
    _check_rows(t, X, D, one, t["G"][[n - 1]], t["X0"], t["P"])
    # the default threshold blanks this file: individual cor_pred is 0.33 - 0.42 here
    blank = ba.bed_ancestry(gb, t["X0"], t["P"], t["corr"], ind_row=rows)
    assert np.isnan(np.asarray(blank)[blank.cor_pred < 0.6]).all()


# ---- G6 ----------------------------------------------------------------------------------------------------------------
def test_bed_ancestry_missing_values(ba):
    t = cases.missing_tables()
    G, X0, P, corr = t["G"], t["X0"], t["P"], t["corr"]
    assert np.isnan(G).any()
    from bigsnpr_amd.ancestry import nearPD
    X = P.T @ X0
    D, ok = nearPD(X.T @ X)
    assert ok
    c = X0.mean(axis=1)
    Gf = np.where(np.isnan(G), 2.0 * c[None, :], G)               # a missing cell counts as 2 c_j
    want = ref.ancestry_rows(Gf, X0, P, corr, D)
    gb = ba.bed(os.path.join(GOLDEN, "example-missing.bed"))
    res = ba.bed_ancestry(gb, X0, P, corr, min_cor=-1)          # keep every row: on these arbitrary groups cor_pred can be negative
    dall = X.T @ ((P.T @ (Gf.T / 2.0)) * corr[:, None])
    well = np.linalg.cond(D) <= 1e4
    for i in range(G.shape[0]):
        same_minimiser(D, dall[:, i], res.unrounded[i], want["w"][i], True, i)
    if well:
        assert np.abs(res.unrounded - want["w"]).max() <= 1e-10
    assert np.abs(res.cor_each - want["cor_each"]).max() <= 1e-10
    assert np.abs(res.cor_pred - want["cor_pred"]).max() <= 1e-10
    rows = np.array([5, 0, 199, 64, 65])
    sub = ba.bed_ancestry(gb, X0, P, corr, ind_row=rows, min_cor=-1)
    assert np.array_equal(sub.unrounded, res.unrounded[rows])
    assert np.array_equal(sub.cor_each, res.cor_each[rows]) and np.array_equal(sub.cor_pred, res.cor_pred[rows])
