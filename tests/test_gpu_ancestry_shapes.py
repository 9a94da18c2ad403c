"""snp_ancestry_summary / bed_ancestry on the device where tests/test_gpu_ancestry.py does not reach: a correction that is
not all ones, the whole per-problem path of k_anc_qp (d formed on the device, l / xf through strides and offsets, cor_one)
at every group width, the chunked frequency columns and two slabs feeding programs, sum_to_one = False, host matrices
through the raw entry, and row / column selections on a .bed image and on an FBM.code256.  Inputs and their claims:
tests/ancestry_cases.py (the shape sweep) and tests/test_ancestry_cpu.py (C5), which holds the CPU statement to the
definition on the same inputs.  Tolerances are those of tests/test_gpu_ancestry.py.  cor_pred is compared with the
statement's number on the problems the statement itself determines (cases.twin_settled: all but some columns of the two
tables with cond(Dmat) = 1e8, where one rounding of its input moves the statement's own cor_pred by 2.4e-10; the device
differed from it by 2.3e-10 there), and with np.corrcoef on the device's own w everywhere.
Measured on one MI355X: worst KKT residual 5.1e-5 tol_kkt, worst correlation error 2.1e-14, the file in 2.8 s."""
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
import king_cases  # noqa: E402

pytestmark = pytest.mark.gpu
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
FIELDS = ("unrounded", "cor_each", "cor_pred", "steps")
_cache = {}


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def dmat(ba, X0, P):
    """Dmat as the mirror forms it: nearPD of X'X, X = P'X0 from the device's moment pass: both sides solve one D"""
    from bigsnpr_amd.ancestry import _dmat
    D = _dmat(ba.ancestry_moments(P, X0)["PtX0"])
    return D, np.linalg.cond(D) <= 1e4


def sweep_dmat(ba, K, L, na):
    if (K, L, na) not in _cache:
        t = cases.sweep_tables(K, L, na)
        _cache[(K, L, na)] = dmat(ba, t["X0"], t["P"])
    return _cache[(K, L, na)]


def codes_of(G):
    return np.where(np.isnan(G), 3, G).astype(np.uint8)


def bed_handle(ba, G):
    n, m = G.shape
    return ba.bed.from_payload(king_cases.encode_payload(codes_of(G)), n, m)


def rows_of(want, sel):
    return {k: v[sel] for k, v in want.items()}


def equal(a, b, what):
    for k in FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=k != "steps"), (what, k)


def hold(t, D, well, F, got, want, settled, s1, what):
    """a device result (B problems; F: their frequency columns, M x B) against the statement's on the same D, and against
    the definition.  settled: the problems whose cor_pred the statement itself determines (cases.twin_settled); on the others
    cor_pred is held to np.corrcoef on the device's own w alone.  Returns (worst KKT residual / tol_kkt, worst correlation
    error against np.corrcoef)."""
    X0 = t["X0"]
    B, K = F.shape[1], X0.shape[1]
    w = got.unrounded
    assert w.shape == (B, K) and got.cor_each.shape == (B, K) and got.cor_pred.shape == (B,) and got.steps.shape == (B,)
    assert (got.steps >= 0).all() and (want["steps"] >= 0).all()
    d = cases.definition_d(t, F)
    # the mirror blanks a row whose cor_pred is not >= min_cor; with min_cor = -1 that is a NaN alone: a prediction
    # without variance, w = 0 (K = 1 under sum w <= 1 with d <= 0)
    blank = np.isnan(want["cor_pred"])
    assert np.array_equal(np.isnan(got.cor_pred), blank), (what, got.cor_pred, want["cor_pred"])
    assert np.isnan(w[blank]).all() and (want["w"][blank] == 0).all(), what
    kept = np.flatnonzero(~blank)
    ratio = 0.0
    for b in kept:
        ratio = max(ratio, cases.same_minimiser(D, d[:, b], w[b], want["w"][b], s1, what + (b,)))
    if well and kept.size:
        assert np.abs(w[kept] - want["w"][kept]).max() <= 1e-10, (what, np.abs(w[kept] - want["w"][kept]).max())
    assert np.array_equal(np.asarray(got)[kept], np.round(w[kept], 7))
    cases.assert_correlations(got.cor_each, got.cor_pred[settled], want["cor_each"], want["cor_pred"][settled], what)
    each, pred = cases.corrcoef_reference(X0, F, np.where(blank[:, None], 0.0, w))
    cases.assert_correlations(got.cor_each, got.cor_pred, each, pred, what)
    err = np.abs(got.cor_each - each).max()
    if kept.size:
        err = max(err, np.abs(got.cor_pred[kept] - pred[kept]).max())
    return ratio, err


def report(what, worst):
    print("%s: worst KKT residual / tol_kkt = %.3g, worst correlation error = %.3g" % (what, worst[0], worst[1]))


SWEEP = pytest.mark.parametrize("K,L", cases.SHAPE_SWEEP)
BOTH = pytest.mark.parametrize("s1", [True, False], ids=["sum_is_one", "sum_at_most_one"])


# ---- S1: the summary path at every group width -----------------------------------------------------------------------------
@BOTH
@SWEEP
def test_summary_every_width(ba, K, L, s1):
    t = cases.sweep_tables(K, L)
    D, well = sweep_dmat(ba, K, L, 0.0)
    counts = cases.sweep_counts(K)
    Fall = cases.frequency_columns(t, counts[-1], cases.SWEEP_SEED[(K, L)])
    twin = lambda A: ref.ancestry_summary(A, t["X0"], t["P"], t["corr"], D, s1)   # noqa: E731
    want, settled = twin(Fall), cases.twin_settled(twin, Fall)
    worst = (0.0, 0.0)
    for B in counts:
        F = np.asfortranarray(Fall[:, :B])          # column b is a function of (seed, b) alone
        got = ba.snp_ancestry_summary(F, t["X0"], t["P"], t["corr"], min_cor=-1, sum_to_one=s1)
        worst = np.maximum(worst, hold(t, D, well, F, got, rows_of(want, slice(0, B)), settled[:B], s1, (K, L, s1, B)))
    report("S1 K %d L %d sum_to_one %d" % (K, L, s1), worst)


# ---- S2: chunked frequency columns feed the programs ---------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("K,L,B", [(60, 64, 9), (32, 17, 40)])      # launches of 4, 4, 1 and of 32, 8 columns
def test_summary_chunked_columns(ba, K, L, B, s1):
    t = cases.synthetic_tables(L + 6, 301, K, L, 500 + K)
    D, well = dmat(ba, t["X0"], t["P"])
    F = cases.frequency_columns(t, B, 600 + K)
    got = ba.snp_ancestry_summary(F, t["X0"], t["P"], t["corr"], min_cor=-1, sum_to_one=s1)
    twin = lambda A: ref.ancestry_summary(A, t["X0"], t["P"], t["corr"], D, s1)   # noqa: E731
    want, settled = twin(F), cases.twin_settled(twin, F)
    report("S2 K %d L %d B %d sum_to_one %d" % (K, L, B, s1), hold(t, D, well, F, got, want, settled, s1, (K, L, B, s1)))
    for b in range(B):                              # a column depends on that column alone
        one = ba.snp_ancestry_summary(np.asfortranarray(F[:, b:b + 1]), t["X0"], t["P"], t["corr"], min_cor=-1, sum_to_one=s1)
        for k in FIELDS:
            assert np.array_equal(getattr(one, k)[0], getattr(got, k)[b], equal_nan=k != "steps"), (K, L, b, k)


# ---- S3: two slabs feed the programs -------------------------------------------------------------------------------------
def test_summary_two_slabs(ba, monkeypatch):
    K, L, B = 9, 4, 5
    t = cases.synthetic_tables(L + 6, ref.slab_rows() + 1, K, L, 31)
    F = cases.frequency_columns(t, B, 32)
    for S in (None, 3):
        if S is None:
            monkeypatch.delenv("BSN_ANC_SLABS", raising=False)
        else:
            monkeypatch.setenv("BSN_ANC_SLABS", str(S))
        D, well = dmat(ba, t["X0"], t["P"])
        twin = lambda A: ref.ancestry_summary(A, t["X0"], t["P"], t["corr"], D, True)   # noqa: E731
        want, settled = twin(F), cases.twin_settled(twin, F)
        got = ba.snp_ancestry_summary(F, t["X0"], t["P"], t["corr"], min_cor=-1)
        report("S3 slabs %s" % S, hold(t, D, well, F, got, want, settled, True, (S,)))
        equal(ba.snp_ancestry_summary(F, t["X0"], t["P"], t["corr"], min_cor=-1), got, S)          # two runs: equal bits


# ---- S4: host matrices through the raw entry ---------------------------------------------------------------------------------
@BOTH
def test_summary_host_matrices(ba, s1):
    K, L, B = 16, 20, 9
    t = cases.sweep_tables(K, L)
    D, _ = sweep_dmat(ba, K, L, 0.0)
    M = t["X0"].shape[0]
    F = cases.frequency_columns(t, B, 41)
    res = ba.snp_ancestry_summary(F, t["X0"], t["P"], t["corr"], min_cor=-1, sum_to_one=s1)      # device-resident matrices
    assert not np.isnan(res.cor_pred).any()

    def padded(a, ld):
        out = np.full((ld, a.shape[1]), np.nan, order="F")
        out[:M] = a
        return out
    Fp, Xp, Pp = padded(F, M + 7), padded(t["X0"], M + 3), padded(t["P"], M + 5)
    p = lambda a: a.ctypes.data_as(f64p)   # noqa: E731
    corr = np.ascontiguousarray(t["corr"])
    for nb in (B, 0):
        w, ce = np.full((B, K), 7.0, order="F"), np.full((B, K), 7.0, order="F")
        cp, steps = np.full(B, 7.0), np.full(B, 7, dtype=np.int32)
        rc = ba.load().bsn_ancestry_summary(p(Fp), M + 7, nb, p(Xp), M + 3, p(Pp), M + 5, p(corr), M, L, K, p(D), int(s1), 0, p(w),
                                            p(ce), p(cp), steps.ctypes.data_as(i32p))
        assert rc == 0
        if nb == 0:                                 # no column: nothing is touched
            assert (w == 7.0).all() and (ce == 7.0).all() and (cp == 7.0).all() and (steps == 7).all()
        else:
            assert np.array_equal(w, res.unrounded) and np.array_equal(ce, res.cor_each)
            assert np.array_equal(cp, res.cor_pred) and np.array_equal(steps, res.steps)


# ---- S5: bed_ancestry at every group width -----------------------------------------------------------------------------------
@BOTH
@SWEEP
def test_bed_ancestry_every_width(ba, K, L, s1):
    t = cases.sweep_tables(K, L, 0.02)
    assert np.isnan(t["G"]).any()
    D, well = sweep_dmat(ba, K, L, 0.02)
    counts = cases.sweep_counts(K)
    Gf = cases.fill_missing(t["G"], t["X0"])[:counts[-1]]
    twin = lambda A: ref.ancestry_rows(A, t["X0"], t["P"], t["corr"], D, s1)   # noqa: E731
    want, settled = twin(Gf), cases.twin_settled(twin, Gf)
    gb = bed_handle(ba, t["G"])
    worst = (0.0, 0.0)
    for nb in counts:
        got = ba.bed_ancestry(gb, t["X0"], t["P"], t["corr"], ind_row=np.arange(nb), min_cor=-1, sum_to_one=s1)
        F = np.asfortranarray(Gf[:nb].T / 2.0)
        worst = np.maximum(worst, hold(t, D, well, F, got, rows_of(want, slice(0, nb)), settled[:nb], s1, (K, L, s1, nb)))
    report("S5 K %d L %d sum_to_one %d" % (K, L, s1), worst)


# ---- S6, S7: selections ------------------------------------------------------------------------------------------------------
SEL_K, SEL_L = 17, 20


def selection_lists():
    n, m = cases.sweep_dims(SEL_K, SEL_L)
    rng = np.random.default_rng(66)
    rows = rng.permutation(np.concatenate([np.arange(n), rng.integers(0, n, size=9)]))      # unsorted, repeats, longer than the image
    assert rows.size > n and np.unique(rows).size < rows.size
    return rows, [None, np.arange(1, m, 3), rng.permutation(m)[:200]]


def selections(ba, obj, s1):
    """[(name, columns, rows or None, result)]: per column list, every row of the image and the row list"""
    t = cases.sweep_tables(SEL_K, SEL_L, 0.02)
    rows, col_lists = selection_lists()
    out = []
    for name, ic in zip(("all columns", "strided", "permuted"), col_lists):
        X0, P = (t["X0"], t["P"]) if ic is None else (np.asfortranarray(t["X0"][ic]), np.asfortranarray(t["P"][ic]))
        for ir in (None, rows):
            out.append((name, ic, ir, ba.bed_ancestry(obj, X0, P, t["corr"], ind_row=ir, ind_col=ic, min_cor=-1, sum_to_one=s1)))
    return out


@BOTH
def test_bed_ancestry_selections(ba, s1):
    t = cases.sweep_tables(SEL_K, SEL_L, 0.02)
    rows = selection_lists()[0]
    full = {}
    worst = (0.0, 0.0)
    for name, ic, ir, got in selections(ba, bed_handle(ba, t["G"]), s1):
        ts = t if ic is None else dict(G=t["G"][:, ic], X0=np.asfortranarray(t["X0"][ic]), P=np.asfortranarray(t["P"][ic]), corr=t["corr"])
        if name not in _cache:
            _cache[name] = dmat(ba, ts["X0"], ts["P"])
        D, well = _cache[name]
        Gf = cases.fill_missing(ts["G"], ts["X0"])
        Gf = Gf if ir is None else Gf[ir]
        twin = lambda A: ref.ancestry_rows(A, ts["X0"], ts["P"], ts["corr"], D, s1)   # noqa: E731
        want, settled = twin(Gf), cases.twin_settled(twin, Gf)
        assert settled.all()
        worst = np.maximum(worst, hold(ts, D, well, np.asfortranarray(Gf.T / 2.0), got, want, settled, s1, (name, ir is None, s1)))
        if ir is None:
            full[name] = got
            continue
        for k in FIELDS:                            # a row depends on that row alone: the sub-selection, and both copies of a repeat
            assert np.array_equal(getattr(got, k), getattr(full[name], k)[rows], equal_nan=k != "steps"), (name, k)
        first = {r: np.flatnonzero(rows == r)[0] for r in rows}
        for i, r in enumerate(rows):
            for k in FIELDS:
                assert np.array_equal(getattr(got, k)[i], getattr(got, k)[first[r]], equal_nan=k != "steps"), (name, i, k)
    report("S6 sum_to_one %d" % s1, worst)


@BOTH
def test_fbm_code256_selections(ba, s1):
    """An FBM.code256 whose table decodes to 0 / 1 / 2 / NA becomes the same 2-bit image as a .bed payload and takes the same
    kernels as long as the selected variants hold a missing value (an FBM knows its missing counts from creation; the
    product drops the missing-value plane only when every selected variant is complete): equal bits are asked."""
    t = cases.sweep_tables(SEL_K, SEL_L, 0.02)
    for ic in selection_lists()[1]:
        assert np.isnan(t["G"] if ic is None else t["G"][:, ic]).any()
    fbm = ba.FBM_code256(codes_of(t["G"]))          # CODE_012: codes 0, 1, 2; 3 decodes to NA
    assert fbm.bits == 2
    for (name, _, ir, a), (_, _, _, b) in zip(selections(ba, fbm, s1), selections(ba, bed_handle(ba, t["G"]), s1)):
        equal(a, b, (name, ir is None))
