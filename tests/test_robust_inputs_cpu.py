"""The inputs of tests/test_gpu_robust_kernels.py (tests/helpers/robust_inputs.py) without a GPU: a wrong kernel of
bigsnpr_amd/csrc/robust.hip cannot pass on them.  The eight passes of the radix select are restated in numpy with named mutants;
every mutant moves the median of one of the device test's columns, while on the kind of data the suite fed the select before
(normal values) the lower passes never choose and a mutant of them is invisible.  The medcouple inputs reach the second turn of
the grid-stride loops with something to count, the hard rejection of the dist_ogk inputs has no borderline row, and the
long-double restatements agree with the oracle's independent ones."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import robust_inputs as ri  # noqa: E402


def _same(a, b):
    """the same double (the two zeros are one value: a sort does not order them)"""
    return a == b


def test_generators_are_what_they_say():
    b = ri.low_bytes(5000, 1.5).view(np.uint64)
    assert np.unique(b >> np.uint64(32)).size == 1 and np.unique(b & np.uint64(0xFFFFFFFF)).size > 4990
    assert np.all(ri.low_bytes(100, 1.5, negate=True) < 0)
    b = ri.every_pass(40000).view(np.uint64)
    for shift in range(0, 64, 8):
        assert np.unique((b >> np.uint64(shift)) & np.uint64(255)).size == 4
    b = ri.one_byte(5000).view(np.uint64)
    assert np.unique(b >> np.uint64(8)).size == 1 and np.unique(b).size == 256
    x = ri.around_zero(5000)
    assert np.abs(x).max() == 6 * 2.0 ** -1074 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    for m in ri.MEDIAN_M:
        X = ri.median_matrix(m, 33)
        assert np.all(np.isfinite(X)) and X.shape == (m, 33)
        np.testing.assert_array_equal(X[:, :7], ri.median_matrix(m, 7))
        if m > 300:
            assert all(not np.array_equal(X[:, a], X[:, b]) for a in range(33) for b in range(a))
    buf = ri.padded(np.arange(6.0).reshape(3, 2), 5)
    np.testing.assert_array_equal(buf, [0, 2, 4, np.nan, np.nan, 1, 3, 5, np.nan, np.nan])
    body, pad = ri.unpadded(buf, 3, 5, 2)
    assert np.array_equal(body, np.arange(6.0).reshape(3, 2)) and np.isnan(pad).all() and pad.shape == (2, 2)


def test_every_pass_chooses_at_every_pass():
    """at m = 40 000 the bucket of the median holds about 10 000, 2 500, 625, 156, 39, 10, 2, 1 keys over the passes: every
    pass sees several occupied bins, and (over the two middle ranks) keys below the chosen one down to the lowest passes"""
    x = ri.every_pass(40000)
    tr_lo, tr_hi = [], []
    ri.select_emulated(x, 19999, trace=tr_lo)
    ri.select_emulated(x, 20000, trace=tr_hi)
    in_bin = [t[1] for t in tr_lo]
    print("keys in the chosen bin per pass:", in_bin)
    for got, want in zip(in_bin, (10000, 2500, 625, 156, 39, 10, 2.4, 0.6)):
        assert want / 3 < got < want * 3 + 2
    assert all(t[2] >= 2 for t in tr_lo[:7])                       # occupied bins among the matching keys
    assert sum(t[3] > 0 for t in tr_lo[4:] + tr_hi[4:]) >= 3       # below > 0 in the low four passes
    # low_bytes: the upper four passes have nothing to choose, the lower four everything
    tr = []
    ri.select_emulated(ri.low_bytes(40001, 1.5), 20000, trace=tr)
    assert [t[2] for t in tr[:4]] == [1, 1, 1, 1] and tr[4][2] == 256 and tr[5][2] > 50 and tr[4][3] > 0 and tr[5][3] > 0


@pytest.mark.parametrize("m", ri.MEDIAN_M)
def test_the_emulation_is_the_exact_median(m):
    """on every column the device test uses, with and without a centre, odd and even m"""
    X = ri.median_matrix(m, 33)
    med = ri.exact_medians(X)
    for c in range(33 if m <= 16385 else 7):
        assert _same(ri.median_emulated(X[:, c]), ri.exact_median(X[:, c])) and _same(med[c], ri.exact_median(X[:, c]))
        assert _same(ri.median_emulated(np.abs(X[:, c] - med[c])), ri.exact_mad(X[:, c], med[c]))
        # exchanging the two middle ranks is no mutant: the same bits
        assert _same(ri.median_emulated(X[:, c], "ranks_swapped"), med[c])
    np.testing.assert_array_equal(ri.exact_medians(X, med), [ri.exact_mad(X[:, c], med[c]) for c in range(33)])


def _caught_by(mutant):
    """the (m, column, with centre) of the device test's inputs on which the mutant returns another median"""
    hits = []
    for m in ri.MEDIAN_M[::-1]:
        X = ri.median_matrix(m, 7)
        med = ri.exact_medians(X)
        for c in range(7):
            if not _same(ri.median_emulated(X[:, c], mutant), med[c]):
                hits.append((m, c, False))
            elif not _same(ri.median_emulated(np.abs(X[:, c] - med[c]), mutant), ri.exact_mad(X[:, c], med[c])):
                hits.append((m, c, True))
        if len(hits) >= 3:
            break
    return hits


@pytest.mark.parametrize("mutant", ri.MUTANTS)
def test_every_mutant_of_the_select_is_caught(mutant):
    hits = _caught_by(mutant)
    print(mutant, "caught on (m, column, centre):", hits)
    assert hits, mutant


def test_the_old_inputs_did_not_see_the_low_passes():
    """30 001 normal values, the kind of column the suite fed the select before: the bucket of the median is down to one key
    after three passes, and a select that stops reducing the rank in its four low passes returns the same bits"""
    x = np.random.default_rng(5).normal(size=30001)
    tr = []
    assert ri.select_emulated(x, 15000, trace=tr) == np.sort(x)[15000]
    print("matching keys per pass:", [t[0] for t in tr])
    assert [t[0] for t in tr[3:]] == [1] * 5 and all(t[3] == 0 for t in tr[3:])
    assert ri.median_emulated(x, "rank_kept_low") == ri.exact_median(x)


@pytest.mark.parametrize("kind", ["lognormal", "dyadic"])
def test_medcouple_inputs_reach_the_second_turn(kind):
    up, lo = ri.mc_input(kind)
    assert up.size == ri.MC_NU > ri.MC_TURN and lo.size == ri.MC_NL and np.all(np.diff(lo) >= 0) and lo[0] > 0 and up.min() > 0
    for t in ri.MC_T:
        tail, total = ri.mc_count_ref(up, lo, t, first=ri.MC_TURN), ri.mc_count_ref(up, lo, t)
        assert 0 < tail < total < up.size * lo.size, (t, tail, total)
    u = up[ri.MC_TURN:]                                             # the definition, on a slice small enough for all pairs
    with np.errstate(all="ignore"):
        h = (u[:, None] - lo[None, :]) / (u[:, None] + lo[None, :])
    if kind == "dyadic":                                            # (exact at t = 0 on the grid)
        assert ri.mc_count_ref(u, lo, 0.0) == int((h <= 0).sum())
    else:
        for t in ri.MC_T:                                           # rounding may move a pair across the bound, hardly ever
            assert abs(ri.mc_count_ref(u, lo, t) - int((h <= t).sum())) <= 2
    for a, b in ri.MC_WINDOWS[kind]:
        tail, whole = ri.mc_window_ref(up, lo, a, b, first=ri.MC_TURN), ri.mc_window_ref(up, lo, a, b)
        print(kind, (a, b), "values:", whole.size, "of them from the second turn:", tail.size)
        assert 1 <= tail.size < whole.size <= 1500000
        assert whole.size == ri.mc_count_ref(up, lo, b) - ri.mc_count_ref(up, lo, a)
        assert whole[0] > a - 1e-12 and whole[-1] <= b + 1e-12
    if kind == "dyadic":
        assert np.isin(up, lo).mean() > 0.1 and np.any(np.diff(lo) == 0)        # thresholds ON values of lo, ties in lo
        assert 0.0 in ri.mc_window_ref(up, lo, *ri.MC_WINDOWS[kind][0])         # h = 0 belongs to (a, 0] ...
        assert ri.mc_window_ref(up, lo, *ri.MC_WINDOWS[kind][1])[0] > 0         # ... and not to (0, b]


def _cut_ratio(p, beta=0.9):
    from scipy.stats import chi2
    return float(chi2.ppf(beta, p) / chi2.ppf(0.5, p))


@pytest.mark.parametrize("p", ri.OGK_P)
def test_no_borderline_row_in_the_hard_rejection(p):
    """n_kept is compared exactly on the device: no row's wdist / d0 within 1e-6 of 1, whatever the number of rounds.  Also
    how far the reference itself moves when every entry of U moves by one relative 2^-52 (printed: the yardstick the device
    test falls back to where rtol 1e-9 has never been measured)."""
    U = ri.ogk_input(p)
    ref = ri.dist_ogk_ref(U, _cut_ratio(p))
    for it in ri.OGK_NITER:
        r = ref[it]
        print("p = %d, niter = %d: n_kept = %d of %d, nearest wdist / d0 to 1: %.2e" % (p, it, r["n_kept"], U.shape[0], r["margin"]))
        assert r["margin"] > 1e-6 and U.shape[0] // 2 <= r["n_kept"] < U.shape[0]
        assert np.all(np.isfinite(r["dist"])) and r["dist"].min() >= 0
    if p <= 33:
        moved = ri.dist_ogk_ref(ri.one_ulp_noise(U), _cut_ratio(p))
        for it in ri.OGK_NITER:
            rel = np.abs(moved[it]["dist"] / ref[it]["dist"] - 1).max()
            print("p = %d, niter = %d: one-ulp noise on U moves the reference by %.2e (relative)" % (p, it, rel))
            assert moved[it]["n_kept"] == ref[it]["n_kept"]


def test_the_restatements_agree_with_the_oracle():
    """scale and rolling mean in np.longdouble against oracle/autosvd_oracle.py's plain loops, ordinary data, 1e-12; the
    whole dist_ogk loop against the oracle's and the product's host path at the device test's tolerance"""
    from oracle import autosvd_oracle as ao
    from bigsnpr_amd import autosvd as prod
    rng = np.random.default_rng(31)
    for m in (1001, 1000, 2):
        x = rng.standard_t(3, size=m) * 2.5 + 1.0
        mu, s = ri.tau2_ref(x)
        omu, osc = ao._tau_scale(x)
        np.testing.assert_allclose([mu, s], [omu, osc], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose([mu, s], prod.scale_tau2(x, mu_too=True), rtol=1e-12, atol=1e-14)
    assert ri.tau2_ref(np.array([2.0, 2.0, 2.0, 2.0, 7.0])) == (2.0, 0.0) and ri.tau2_ref(np.array([4.0])) == (4.0, 0.0)
    for c1, c2 in ri.TAU2_CONSTANTS:                                # the constants reach both stages
        x = rng.normal(size=501)
        np.testing.assert_allclose(ri.tau2_ref(x, c1, c2), prod.scale_tau2(x, c1, c2, mu_too=True), rtol=1e-12, atol=1e-14)
    assert abs(ri.erho_of(3.0 * ri.Q75) - prod._erho(3.0 * ri.Q75)) < 1e-15
    for n, size in ((200, 50), (40, 3), (200, 7)):
        x = rng.lognormal(size=n)
        w = prod._rollmean_weights(size)[0]
        np.testing.assert_allclose(ri.rollmean_ref(x, w).astype(np.float64), ao.rollmean(x, size), rtol=1e-12)
    x = rng.lognormal(size=300)                                     # groups: every group on its own
    w = ri.rollmean_weights(21)
    got = ri.rollmean_ref(x, w, (0, 5, 6, 200, 300))
    for a, b in ((0, 5), (5, 6), (6, 200), (200, 300)):
        np.testing.assert_array_equal(got[a:b], ri.rollmean_ref(x[a:b], w))
    U = ri.ogk_input(5, 601)
    ref = ri.dist_ogk_ref(U, _cut_ratio(5), niters=(2,))[2]
    np.testing.assert_allclose(ref["dist"], ao.dist_ogk(U), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(ref["dist"], prod.dist_ogk(U), rtol=1e-9, atol=1e-12)
    # the plain products
    Z, E = ri.product_matrix(50, 7), rng.normal(size=(7, 7))
    np.testing.assert_allclose(ri.rotate_ref(Z, E)[0].astype(np.float64), Z @ E, rtol=1e-12, atol=1e-13)
    mu, sig = rng.normal(size=7), rng.uniform(0.5, 2, size=7)
    np.testing.assert_allclose(ri.wdist_ref(Z, mu, sig).astype(np.float64), (((Z - mu) / sig) ** 2).sum(1), rtol=1e-13)
    P = E @ E.T
    np.testing.assert_allclose(ri.mahalanobis_ref(Z, mu, P).astype(np.float64), np.einsum("ij,jk,ik->i", Z - mu, P, Z - mu), rtol=1e-12)
