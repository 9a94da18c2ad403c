"""snp_ancestry_summary without a device: the CPU statement of the quadratic program (tests/native/ancestry_ref.cpp over
bigsnpr_amd/csrc/qp_step.hpp) against the program's definition, nearPD against its properties, a planted mixture on the
golden example.bed, the host mirror's checks and messages, and the statement on the synthetic tables of the shape sweep
(a correction that is not all ones).  tests/test_gpu_ancestry.py and tests/test_gpu_ancestry_shapes.py hold the kernels to
that statement."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ancestry_cases as cases  # noqa: E402
import ancestry_ref as ref  # noqa: E402
from bigsnpr_amd import ancestry as anc  # noqa: E402

QP_CASES = cases.qp_cases(anc.nearPD)


# ---- C1: the statement's program against the definition ---------------------------------------------------------------------
def test_cap_is_the_one_the_cases_assume():
    assert ref.max_k() == cases.CAP == anc.MAX_K


@pytest.mark.parametrize("case", QP_CASES, ids=[c[0] for c in QP_CASES])
def test_qp_against_the_definition(case):
    name, D, d, s1, w_known = case
    r = ref.qp_simplex(D, d, s1)
    w = r["w"][0]
    assert r["n_failed"] == 0 and 0 <= r["steps"][0] <= ref.load().qp_iter_cap(d.size)
    ratio = cases.check_solution(D, d, w, s1, name)
    print("%s: worst KKT residual / tol_kkt = %.3g, steps %d" % (name, ratio, r["steps"][0]))
    f, fs = cases.objective(D, d, w), cases.objective(D, d, cases.slsqp(D, d, s1))
    assert f <= fs + 1e-9 * (1.0 + abs(fs)), (name, f, fs)
    if w_known is not None:
        assert np.abs(w - w_known).max() <= 1e-9, (name, w, w_known)


def test_qp_shapes_of_the_case_list():
    names = [c[0] for c in QP_CASES]
    w = {c[0]: ref.qp_simplex(c[1], c[2], c[3])["w"][0] for c in QP_CASES}
    assert (w["interior"] > 0).all()                                   # no active bound
    assert (w["vertex"] == 0).sum() == w["vertex"].size - 1            # K - 1 bounds active
    assert abs(w["below_one"].sum() - 0.5) < 1e-9                      # the sum constraint inactive
    assert (w["all_negative"] == 0).all()
    assert "twins_True" in names and "cap_True" in names


def test_qp_refusals_and_nan():
    D = np.eye(cases.CAP + 1)
    with pytest.raises(ref.Refused, match="above the cap"):
        ref.qp_simplex(D, np.zeros(cases.CAP + 1))
    with pytest.raises(ref.Refused, match="Cholesky"):
        ref.qp_simplex(np.array([[1.0, 2.0], [2.0, 1.0]]), np.zeros(2))
    D = np.eye(3) + 0.1
    d = np.array([[0.3, np.nan, 0.1], [0.2, 0.5, np.inf], [0.1, 0.2, 0.3]]).T
    r = ref.qp_simplex(D, d)
    assert np.isnan(r["w"][:2]).all() and list(r["steps"][:2]) == [-1, -1] and r["n_failed"] == 0
    cases.check_solution(D, d[:, 2], r["w"][2], True)


@pytest.mark.parametrize("K", [2, 9, 19, 33])
def test_qp_batches_ill_conditioned(K):
    # D = nearPD of a singular X'X (condition about 1e8), d in the range of X': the regime of 16 loadings and 21 groups
    D, d = cases.problem_batch(K, 40, 100 + K, anc.nearPD)
    for s1 in (True, False):
        r = ref.qp_simplex(D, d, s1)
        assert r["n_failed"] == 0
        for b in range(d.shape[1]):
            cases.check_solution(D, d[:, b], r["w"][b], s1, (K, s1, b))


def test_header_under_a_sanitizer(tmp_path):
    exe = str(tmp_path / "ancestry_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-ffp-contract=off", "-std=c++17",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "bigsnpr_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "native"),
                           os.path.join(ROOT, "tests", "native", "ancestry_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks held" in out.stdout


# ---- C2: nearPD -----------------------------------------------------------------------------------------------------------
def test_nearpd_properties():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(10, 19))
    S = X.T @ X                                    # rank 10 of 19
    D, ok = anc.nearPD(S)
    assert ok and np.array_equal(D, D.T)
    ev = np.linalg.eigvalsh(D)
    assert ev[0] >= 0.99 * 1e-8 * ev[-1]
    A = rng.normal(size=(30, 8))
    W = A.T @ A                                    # well conditioned
    Dw, okw = anc.nearPD(W)
    assert okw and np.abs(Dw - W).max() <= 1e-12 * np.abs(W).max()
    Dw2, okw2 = anc.nearPD(Dw)                     # twice: nothing changes
    assert okw2 and np.abs(Dw2 - Dw).max() <= 1e-12 * np.abs(Dw).max()
    # On the result of a SINGULAR input the rule itself is idempotent to the order of posd.tol only, not to 1e-12: the
    # eigenvalues that the last step raised to Eps = posd.tol lambda_1 lie below eig.tol lambda_1, so a second
    # application drops them (a change of at most Eps in the 2-norm), raises them to Eps again (at most Eps) and rescales
    # the diagonal to that of the truncated matrix (at most Eps more): 3 Eps in all.  Measured here: 2.1e-8 lambda_1.
    D2, ok2 = anc.nearPD(D)
    change = np.linalg.norm(D2 - D, 2)
    print("nearPD twice on a singular input: change %.3g lambda_1" % (change / ev[-1]))
    assert ok2 and change <= 3.0 * 1e-8 * ev[-1]
    with pytest.raises(ValueError):
        anc.nearPD(-np.eye(3))


# ---- C3: a planted mixture on example.bed ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ex25():
    return cases.example_tables(25)


@pytest.fixture(scope="module")
def ex10():
    return cases.example_tables(10)


def _dmat(t):
    X = t["P"].T @ t["X0"]
    D, ok = anc.nearPD(X.T @ X)
    assert ok
    return X, D


def test_planted_mixture_full_rank(ex25):
    t = ex25
    assert t["G"].shape == (517, 4542) and not np.isnan(t["G"]).any()
    X, D = _dmat(t)
    assert np.linalg.cond(D) < 1e5
    r = ref.ancestry_summary(t["freq"], t["X0"], t["P"], t["corr"], D)
    assert np.abs(r["w"][0] - t["wt"]).max() <= 1e-7
    assert r["cor_pred"][0] > 1 - 1e-9
    want = [np.corrcoef(t["X0"][:, k], t["freq"])[0, 1] for k in range(19)]
    assert np.abs(r["cor_each"][0] - want).max() <= 1e-10


def test_planted_mixture_rank_deficient(ex10):
    t = ex10
    X, D = _dmat(t)
    assert np.linalg.cond(D) > 1e7
    r = ref.ancestry_summary(t["freq"], t["X0"], t["P"], t["corr"], D)
    d = X.T @ ((t["P"].T @ t["freq"]) * t["corr"])
    cases.check_solution(D, d, r["w"][0], True)
    assert r["cor_pred"][0] > 1 - 1e-9


def test_moments_statement_against_numpy(ex10):
    t = ex10
    F = np.stack([t["freq"], 1.0 - t["freq"]], axis=1)
    m = ref.moments(t["P"], t["X0"], F)
    for got, want in ((m["PtX0"], t["P"].T @ t["X0"]), (m["PtF"], t["P"].T @ F), (m["G0"], t["X0"].T @ t["X0"]),
                      (m["X0tF"], t["X0"].T @ F), (m["csX0"], t["X0"].sum(0)), (m["csF"], F.sum(0)), (m["sqF"], (F * F).sum(0))):
        assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max())


def test_rows_statement_against_summary(ex10):
    # a genotype row is the frequency vector g / 2
    t = ex10
    X, D = _dmat(t)
    rows = [0, 100, 516]
    a = ref.ancestry_rows(t["G"][rows], t["X0"], t["P"], t["corr"], D)
    b = ref.ancestry_summary(t["G"][rows].T / 2.0, t["X0"], t["P"], t["corr"], D)
    for k in ("w", "cor_each", "cor_pred"):
        assert np.abs(a[k] - b[k]).max() <= 1e-10, k


# ---- C4: the mirror's checks and messages (all raised before any device work) ----------------------------------------------------
def test_mirror_checks(ex10):
    t = ex10
    f, X0, P, c = t["freq"], t["X0"], t["P"], t["corr"]
    bad = f.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="missing values in 'freq'"):
        anc.snp_ancestry_summary(bad, X0, P, c)
    badX = X0.copy()
    badX[0, 0] = np.nan
    with pytest.raises(ValueError, match="missing values in 'info_freq_ref'"):
        anc.snp_ancestry_summary(f, badX, P, c)
    badP = P.copy()
    badP[0, 0] = np.nan
    with pytest.raises(ValueError, match="missing values in 'projection'"):
        anc.snp_ancestry_summary(f, X0, badP, c)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        anc.snp_ancestry_summary(f[:-1], X0, P, c)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        anc.snp_ancestry_summary(f, X0, P[:-1], c)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        anc.snp_ancestry_summary(f, X0, P, c[:-1])
    with pytest.raises(ValueError, match="Frequencies seem all reversed; switch reference allele"):
        anc.snp_ancestry_summary(1.0 - f, X0, P, c)


def test_mirror_min_cor():
    K = 3
    w = np.full((2, K), 1.0 / 3)
    ce = np.zeros((2, K))
    steps = np.zeros(2, dtype=np.int32)
    ms = np.zeros(3)
    with pytest.raises(ValueError, match="Correlation between frequencies is too low: 0.250; check matching between variants."):
        anc._finish_summary(True, np.zeros(1, bool), w[:1].copy(), ce[:1], np.array([0.25]), steps[:1], None, ms, 0.4)
    with pytest.warns(UserWarning, match="does not perfectly match"):
        out = anc._finish_summary(True, np.zeros(1, bool), w[:1].copy(), ce[:1], np.array([0.9]), steps[:1], ["a", "b", "c"], ms, 0.4)
    assert out.shape == (K,) and out.names == ["a", "b", "c"] and out.cor_pred == 0.9 and isinstance(out, anc.AncestryProportions)
    assert np.array_equal(np.asarray(out), np.round(w[0], 7))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = anc._finish_summary(False, np.array([False, False]), w.copy(), ce, np.array([0.25, 0.995]), steps, None, ms, 0.4)
    assert out.shape == (2, K) and np.isnan(out[0]).all() and np.isfinite(out[1]).all()
    out = anc._finish_summary(False, np.array([False, True]), w.copy(), ce, np.array([0.9, 0.9]), steps, None, ms, 0.4)
    assert np.isfinite(out[0]).all() and np.isnan(out[1]).all()


# ---- C5: the shape sweep (a correction that is not all ones, every group width of the kernel) -----------------------------------
# Under sum_to_one = False the shrunk mixture 0.6 X0 w leaves the sum constraint inactive only where the correction does not
# undo the shrinking: the unconstrained minimiser of such a column sums to 0.6 1'A w, A = Dmat^-1 X' diag(corr) X, and on
# these three tables every column sum of A is above 1 / 0.6 (smallest 2.38, 3.10 and 3.77: most of the K - 1 directions
# between the populations lie at loadings whose correction is 2 and more), so every mixture of the simplex ends at sum w = 1.
# Each group width keeps a table with an inactive sum: (17, 20) and (19, 5) for 32 lanes, (60, 10) for 64.
SUM_ALWAYS_ONE = [(32, 40), (33, 40), (60, 64)]


@functools.lru_cache(maxsize=None)
def sweep_problem(K, L, na, s1):
    """one sweep entry on the twin: the problems the device sweep solves (the frequency columns of the summary path for
    na = 0, the first rows of the image with its missing cells filled for na > 0), Dmat and d by the definition in numpy"""
    t = cases.sweep_tables(K, L, na)
    X = t["P"].T @ t["X0"]
    D, ok = anc.nearPD(X.T @ X)
    assert ok
    B = cases.sweep_counts(K)[-1]
    if na == 0.0:
        F = cases.frequency_columns(t, B, cases.SWEEP_SEED[(K, L)])
        A, twin = F, lambda A: ref.ancestry_summary(A, t["X0"], t["P"], t["corr"], D, s1)   # noqa: E731
    else:
        Gf = cases.fill_missing(t["G"], t["X0"])[:B]
        F = np.asfortranarray(Gf.T / 2.0)
        A, twin = Gf, lambda A: ref.ancestry_rows(A, t["X0"], t["P"], t["corr"], D, s1)   # noqa: E731
    return dict(t=t, D=D, F=F, d=cases.definition_d(t, F), r=twin(A), settled=cases.twin_settled(twin, A))


@pytest.mark.parametrize("s1", [True, False])
@pytest.mark.parametrize("na", [0.0, 0.02], ids=["summary", "rows"])
@pytest.mark.parametrize("K,L", cases.SHAPE_SWEEP)
def test_sweep_against_the_definition(K, L, na, s1):
    p = sweep_problem(K, L, na, s1)
    t, D, F, d, r = p["t"], p["D"], p["F"], p["d"], p["r"]
    B = F.shape[1]
    assert t["corr"].size == L and (np.diff(t["corr"]) > 0).all() and t["corr"][0] == 1.0
    assert not np.isnan(t["X0"]).any() and np.isnan(t["G"]).any() == (na > 0)
    assert (r["steps"] >= 0).all() and (r["steps"] <= ref.load().qp_iter_cap(K)).all()
    worst = max(cases.check_solution(D, d[:, b], r["w"][b], s1, (K, L, na, s1, b)) for b in range(B))
    each, pred = cases.corrcoef_reference(t["X0"], F, r["w"])
    cases.assert_correlations(r["cor_each"], r["cor_pred"], each, pred, (K, L, na, s1))
    ok = ~np.isnan(pred)
    err = max(np.abs(r["cor_each"] - each).max(), np.abs(r["cor_pred"][ok] - pred[ok]).max() if ok.any() else 0.0)
    ones = ref.ancestry_summary(F, t["X0"], t["P"], np.ones(L), D, s1)["w"]
    print("K %d L %d na %g sum_to_one %d: worst KKT residual / tol_kkt = %.3g, worst correlation error %.3g, the correction moves w by "
          "%.3g" % (K, L, na, s1, worst, err, np.abs(r["w"] - ones).max()))
    if K == 1 and not s1:
        # sum w <= 1 alone: w = 0 wherever d <= 0, and the prediction has no variance there
        zero = r["w"][:, 0] == 0
        assert np.array_equal(zero, d[0] <= 0) and np.array_equal(np.isnan(r["cor_pred"]), zero)
    else:
        assert ok.all()


def test_sweep_conditioning():
    cond = {kl: np.linalg.cond(sweep_problem(*kl, 0.0, True)["D"]) for kl in cases.SHAPE_SWEEP}
    print({kl: "%.3g" % c for kl, c in cond.items()})
    for W in (8, 16, 32, 64):
        assert any(c <= 1e4 for (K, L), c in cond.items() if cases.group_width(K) == W), W     # w itself is compared there
    for kl in cases.RANK_DEFICIENT:
        assert cond[kl] > 1e7, (kl, cond[kl])


def test_sweep_sum_constraint_both_ways():
    inactive_at = set()
    for K, L in cases.SHAPE_SWEEP:
        sums = sweep_problem(K, L, 0.0, False)["r"]["w"].sum(axis=1)
        assert (np.abs(sums - 1.0) <= 1e-12).any(), (K, L, sums)
        if (K, L) in SUM_ALWAYS_ONE:
            assert (np.abs(sums - 1.0) <= 1e-12).all(), (K, L, sums)
        else:
            assert (sums < 1.0 - 1e-6).any(), (K, L, sums)
            inactive_at.add(cases.group_width(K))
    assert inactive_at == {8, 16, 32, 64}


def test_sweep_partial_steps_at_every_width():
    # a constraint leaves the active set (the row rotations of R and J) in some problem of the device sweep, at every width
    for W in (8, 16, 32, 64):
        drops = [cases.proven_drops(p["r"]["w"][b], p["r"]["steps"][b])
                 for K, L in cases.SHAPE_SWEEP if cases.group_width(K) == W for na in (0.0, 0.02) for s1 in (True, False)
                 for p in [sweep_problem(K, L, na, s1)] for b in range(p["F"].shape[1])]
        print("%d lanes: most partial steps proven in one problem: %d" % (W, max(drops)))
        assert max(drops) >= 1, W


def test_sweep_generators():
    K, L = 17, 20
    t = cases.sweep_tables(K, L, 0.02)
    n, m = cases.sweep_dims(K, L)
    assert t["G"].shape == (n, m) and t["X0"].shape == (m, K) and t["P"].shape == (m, L) and m % 4 and m % 64
    assert t["X0"].min() >= 0.02 and t["X0"].max() <= 0.98 and 0.005 < np.isnan(t["G"]).mean() < 0.04
    assert abs(t["corr"][-1] - (1.0 + 0.013 * 19 ** 1.5)) < 1e-15
    F9, F4 = cases.frequency_columns(t, 9, 5), cases.frequency_columns(t, 4, 5)
    assert np.array_equal(F9[:, :4], F4) and not np.isnan(F9).any()          # a column depends on (seed, b) alone
    lo, hi = t["X0"].min(axis=1), t["X0"].max(axis=1)
    assert (F9[:, 0] >= lo - 1e-15).all() and (F9[:, 0] <= hi + 1e-15).all()                 # a mixture of the columns of X0
    assert (F9[:, 1] >= 0.6 * lo - 1e-15).all() and (F9[:, 1] <= 0.6 * hi + 1e-15).all()     # shrunk by 0.6
    assert (np.isin(F9[:, 2], [0.0, 0.5, 1.0]) | (F9[:, 2] == t["X0"].mean(axis=1))).all()   # a genotype row / 2
    assert cases.proven_drops(np.array([0.0, 0.5, 0.5]), 6) == 2 and cases.proven_drops(np.array([0.0, 0.0, 1.0]), 3) == 0
    with pytest.raises(AssertionError):
        cases.synthetic_tables(L + 5, 50, 3, L, 1)


def test_sweep_where_the_statement_is_a_reference_for_cor_pred():
    # the device's cor_pred is held to the statement's on the settled problems: all of them, but for some of the tables with L < K
    for K, L in cases.SHAPE_SWEEP:
        for na in (0.0, 0.02):
            for s1 in (True, False):
                p = sweep_problem(K, L, na, s1)
                left = int((~p["settled"]).sum())
                print("K %d L %d na %g sum_to_one %d: %d of %d problems not settled" % (K, L, na, s1, left, p["settled"].size))
                assert left == 0 or (K, L) in cases.RANK_DEFICIENT, (K, L, na, s1, p["settled"])
