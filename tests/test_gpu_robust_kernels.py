"""The kernels of bigsnpr_amd/csrc/robust.hip — the outlier step of snp_autoSVD / bed_autoSVD — where their passes, strides and
loops bite: medians observed directly (bsn_robust_medians) on keys that make every byte pass of the radix select choose,
leading dimensions larger than the column (NaN in the padding rows), 64 columns, the second chunk of the pair scales, the
second turn of the medcouple's grid-stride loops, windows of up to 4095 taps, other constants than the defaults, and the
refusals.  Inputs and references: tests/helpers/robust_inputs.py — exact selection on a sort, np.longdouble restatements;
tests/test_robust_inputs_cpu.py shows without a GPU that a wrong select cannot pass on them.

Tolerances: bit equality for medians, counts, kernel values and n_kept; rtol 1e-12 (atol 1e-14 on mu) for the scales and rtol
1e-9 / atol 1e-12 for the distances, the numbers of tests/test_gpu_autosvd.py; bounds derived from p, the number of taps and
eps = 2^-52 for the plain products and the rolling mean."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import robust_inputs as ri  # noqa: E402

pytestmark = pytest.mark.gpu

LD, EPS, PAD = ri.LD, ri.EPS64, ri.PAD


@pytest.fixture(scope="module")
def lib():
    from bigsnpr_amd import _lib
    return _lib


def _up(lib, X, ld=None):
    """the matrix (or vector) on the device, column-major with leading dimension ld and NaN in the padding rows"""
    X = np.asarray(X, dtype=np.float64)
    m = X.shape[0]
    return lib.DeviceArray.from_numpy(ri.padded(X, m if ld is None else ld))


def _f(lib, a):
    return lib.ptr(a, lib.f64p)


def _refused(lib, rc, text):
    assert rc != 0
    msg = lib.load().bsn_last_error().decode()
    assert text in msg, msg


def _cut_ratio(p, beta=0.9):
    from scipy.stats import chi2
    return float(chi2.ppf(beta, p) / chi2.ppf(0.5, p))


# ---- medians ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ri.MEDIAN_M)
def test_medians_bit_for_bit(lib, m):
    """k_sel_hist + k_sel_pick + k_sel_median through bsn_robust_medians: every column from another generator or seed (a mix-up
    of virtual columns shows), 1 / 7 / 33 columns, ld = m and m + 37, the plain median and the median of |x - centre| (the
    MAD step, and a centre that is not the median).  16 384 is the last size with one turn of the loop at 64 workgroups."""
    L = lib.load()
    X = ri.median_matrix(m, 33)
    med = ri.exact_medians(X)
    other = np.ascontiguousarray(X[0] * (1.0 + 2.0 ** -30))
    want = {None: med, "mad": ri.exact_medians(X, med), "other": ri.exact_medians(X, other)}
    centres = {None: None, "mad": np.ascontiguousarray(med), "other": other}
    for ld in (m, m + PAD):
        d = _up(lib, X, ld)
        for ncol in ri.MEDIAN_NCOL:
            for key, centre in centres.items():
                got = np.full(ncol, -1.0)
                lib.check(L.bsn_robust_medians(d.ptr, m, ld, ncol, _f(lib, centre), _f(lib, got)))
                bad = np.nonzero(~(got == want[key][:ncol]))[0]
                assert np.array_equal(got, want[key][:ncol]), (m, ld, ncol, key, [(int(c), ri.GENERATOR_NAMES[c % 7]) for c in bad])
        lib.check(L.bsn_robust_medians(d.ptr, m, ld, 0, None, None))                   # no columns: nothing to do
        d.free()


# ---- scaleTau2 --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c1,c2", ri.TAU2_CONSTANTS)
@pytest.mark.parametrize("m", [16385, 2, 1])
def test_scale_tau2_other_constants_padded(lib, m, c1, c2):
    """k_tau_sums / k_tau_finish with ld = m + 37 on 33 columns, a MAD-0 column and a constant column between ordinary ones
    (s == 0 exactly, mu the exact median), Erho at c2 = 3, 2 and 1.5, and mu_out = NULL"""
    L = lib.load()
    X = ri.tau2_matrix(m)
    ncol, ld = X.shape[1], m + PAD
    rmu, rs = ri.tau2_ref_cols(X, c1, c2)
    d = _up(lib, X, ld)
    mu, s, s_only = np.full(ncol, np.nan), np.full(ncol, np.nan), np.full(ncol, np.nan)
    lib.check(L.bsn_robust_scale_tau2(d.ptr, m, ld, ncol, c1, c2, _f(lib, mu), _f(lib, s)))
    lib.check(L.bsn_robust_scale_tau2(d.ptr, m, ld, ncol, c1, c2, None, _f(lib, s_only)))
    d.free()
    print("m = %d, c = (%g, %g): max relative difference s %.2e, mu %.2e" % (
        m, c1, c2, np.abs(s / np.where(rs > 0, rs, 1) - (rs > 0)).max(), np.abs((mu - rmu) / np.where(rmu != 0, rmu, 1)).max()))
    np.testing.assert_allclose(mu, rmu, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(s, rs, rtol=1e-12)
    np.testing.assert_array_equal(s_only, s)
    zero = [ri.TAU2_MAD0, ri.TAU2_CONST] if m > 1 else list(range(ncol))
    assert np.all(rs[zero] == 0) and np.all(s[zero] == 0) and np.array_equal(mu[zero], ri.exact_medians(X)[zero])
    if m > 2:
        assert np.all(np.delete(s, zero) > 0)


# ---- pair scales ------------------------------------------------------------------------------------------------------------------

def test_pair_scales_of_64_columns(lib):
    """k_pairs at p = 64: 2 016 pairs, 4 032 columns in one chunk, every pair against scaleTau2 of the float64 sums and
    differences in the documented order; ld = m and m + 37"""
    L = lib.load()
    m, p = 2049, 64
    Z = ri.pair_matrix(m, p)
    pairs = ri.pair_list(p)
    assert len(pairs) == 2016 and pairs[:4] == [(1, 0), (2, 0), (2, 1), (3, 0)] and pairs[-1] == (63, 62)
    rsum, rdiff = ri.pair_scales_ref(Z, pairs)
    for ld in (m, m + PAD):
        d = _up(lib, Z, ld)
        ss, sd = np.full(len(pairs), np.nan), np.full(len(pairs), np.nan)
        lib.check(L.bsn_robust_pair_scales(d.ptr, m, ld, p, 4.5, 3.0, _f(lib, ss), _f(lib, sd)))
        d.free()
        np.testing.assert_allclose(ss, rsum, rtol=1e-12)
        np.testing.assert_allclose(sd, rdiff, rtol=1e-12)


def test_pair_scales_second_chunk(lib):
    """p = 64 at m = 66 577, the smallest m with floor(2^27 / m) = 2 015 < 2 016 pairs: the last pair, (63, 62), is a chunk of
    its own (d_pi.p + q0, s_sum_out[q0 + q]; 2.1 GB of device scratch).  On the host: that pair, the first and the last pair of
    the first chunk and 60 pairs drawn at random; every scale finite and positive."""
    L = lib.load()
    m, p = 66577, 64
    assert (1 << 27) // m == 2015 and (1 << 27) // (m - 1) == 2016
    Z = ri.pair_matrix(m, p)
    pairs = ri.pair_list(p)
    pick = sorted({2015, 0, 2014} | set((1 + np.random.default_rng(3).choice(2013, size=60, replace=False)).tolist()))
    assert len(pick) == 63
    assert pairs[2015] == (63, 62)
    rsum, rdiff = ri.pair_scales_ref(Z, [pairs[q] for q in pick])
    ld = m + PAD
    d = _up(lib, Z, ld)
    ss, sd = np.full(len(pairs), np.nan), np.full(len(pairs), np.nan)
    lib.check(L.bsn_robust_pair_scales(d.ptr, m, ld, p, 4.5, 3.0, _f(lib, ss), _f(lib, sd)))
    d.free()
    assert np.all(np.isfinite(ss)) and np.all(np.isfinite(sd)) and ss.min() > 0 and sd.min() > 0
    np.testing.assert_allclose(ss[pick], rsum, rtol=1e-12)
    np.testing.assert_allclose(sd[pick], rdiff, rtol=1e-12)


# ---- rotate, scale_cols, wdist ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [257, 1025])
@pytest.mark.parametrize("p", [1, 33, 64])
def test_rotate_scale_cols_wdist(lib, p, m):
    """k_rotate (a row of p <= 64 values per thread, E in LDS), k_scale_cols, k_wdist with ld = m and m + 37; the in-place
    kernels leave the padding rows alone.  Bounds, elementwise, against the products in np.longdouble:
      rotate      2 p eps (|Z| |E|): p products and p - 1 additions per entry, first-order worst case p eps / 2;
      scale_cols  eps |ref|: one division;
      wdist       (p + 4) eps sum of the terms: a term ((z - mu) / sig)^2 carries the roundings of the difference and of the
                  quotient twice and its own (5 eps / 2), the sum p - 1 more ((p - 1) eps / 2) — twice the first-order worst case."""
    L = lib.load()
    rng = np.random.default_rng([41, p, m])
    Z = ri.product_matrix(m, p)
    E = np.asfortranarray(rng.normal(size=(p, p)))
    div = rng.uniform(0.3, 3.0, size=p) * rng.choice([-1.0, 1.0], size=p)
    mu, sig = rng.normal(size=p), rng.uniform(0.3, 3.0, size=p)
    rot, rot_abs = ri.rotate_ref(Z, E)
    wd = ri.wdist_ref(Z, mu, sig)
    for ld in (m, m + PAD):
        buf = ri.padded(Z, ld)
        pad_bits = ri.unpadded(buf, m, ld, p)[1].view(np.uint64).copy()
        # wdist
        d = lib.DeviceArray.from_numpy(buf)
        got = np.full(m, np.nan)
        lib.check(L.bsn_robust_wdist(d.ptr, m, ld, p, _f(lib, mu), _f(lib, sig), _f(lib, got)))
        err = np.abs(got.astype(LD) - wd)
        print("p = %d, m = %d, ld = %d: wdist max err / bound %.3f" % (p, m, ld, float((err / ((p + 4) * EPS * wd)).max())))
        assert np.all(err <= (p + 4) * EPS * wd)
        # rotate, in place
        lib.check(L.bsn_robust_rotate(d.ptr, m, ld, p, _f(lib, E)))
        body, pad = ri.unpadded(d.to_numpy().ravel(), m, ld, p)
        err = np.abs(body.astype(LD) - rot)
        print("p = %d, m = %d, ld = %d: rotate max err / bound %.3f" % (p, m, ld, float((err / (2 * p * EPS * rot_abs)).max())))
        assert np.all(err <= 2 * p * EPS * rot_abs)
        assert np.array_equal(pad.view(np.uint64), pad_bits)
        d.free()
        # scale_cols, in place
        d = lib.DeviceArray.from_numpy(buf)
        lib.check(L.bsn_robust_scale_cols(d.ptr, m, ld, p, _f(lib, div)))
        body, pad = ri.unpadded(d.to_numpy().ravel(), m, ld, p)
        ref = Z.astype(LD) / div.astype(LD)
        assert np.all(np.abs(body.astype(LD) - ref) <= EPS * np.abs(ref))
        assert np.array_equal(pad.view(np.uint64), pad_bits)
        d.free()


# ---- dist_ogk ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", ri.OGK_P)
def test_dist_ogk_rounds_columns_and_padding(lib, p):
    """bsn_robust_dist_ogk at p = 1, 33, 64 (k_rotate, k_mahalanobis and the pair scales at their limit), m = 4 097, niter = 0, 1,
    2, ld = m and m + 37 (k_mahalanobis and k_keep_sums read d_U through ld: NaN in the padding), n_kept_out requested: the
    distances against the host loop put together from the long-double pieces (ri.dist_ogk_ref), rtol 1e-9 / atol 1e-12 as in
    tests/test_gpu_autosvd.py, n_kept exactly (no row within 1e-6 of the cut: tests/test_robust_inputs_cpu.py).  Second
    comparators where they are quick (p = 1; their 2 (p + p (p - 1)) scales, one after the other, take 7 s at p = 33 and 25 s at
    p = 64): the product's host path and the oracle's loop.  tests/test_robust_inputs_cpu.py compares all three at p = 5."""
    from bigsnpr_amd import autosvd as prod
    from oracle import autosvd_oracle as orc_a
    L = lib.load()
    U = ri.ogk_input(p)
    m = U.shape[0]
    cut = _cut_ratio(p)
    ref = ri.dist_ogk_ref(U, cut)
    for ld in (m, m + PAD):
        d = _up(lib, U, ld)
        for niter in ri.OGK_NITER:
            got, nk = np.full(m, np.nan), C.c_int64(-1)
            lib.check(L.bsn_robust_dist_ogk(d.ptr, m, ld, p, niter, cut, 4.5, 3.0, _f(lib, got), C.byref(nk)))
            r = ref[niter]
            print("p = %d, ld = %d, niter = %d: n_kept %d (reference %d), max relative difference %.2e"
                  % (p, ld, niter, nk.value, r["n_kept"], np.abs(got / r["dist"] - 1).max()))
            assert nk.value == r["n_kept"]
            np.testing.assert_allclose(got, r["dist"], rtol=1e-9, atol=1e-12)
            if p == 1 and ld == m:
                np.testing.assert_allclose(got, prod.dist_ogk(U, niter), rtol=1e-9, atol=1e-12)
                np.testing.assert_allclose(got, orc_a.dist_ogk(U, niter), rtol=1e-9, atol=1e-12)
        d.free()


# ---- medcouple --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["lognormal", "dyadic"])
def test_mc_count_and_window_past_the_first_turn(lib, kind):
    """k_mc_count / k_mc_window with 262 144 + 300 values of `up`: 1024 workgroups of 256 threads take a second turn for the last
    300, which count at every t and put values into every window (tests/test_robust_inputs_cpu.py).  Counts as integers,
    windows as multisets, and the call over its cap that returns the count only.  "dyadic": all values k / 64, thresholds
    exactly on values of `lo` at t = 0 and at the window bounds 0 — the side = "left" edge."""
    L = lib.load()
    up, lo = ri.mc_input(kind)
    dU, dL = lib.DeviceArray.from_numpy(up), lib.DeviceArray.from_numpy(lo)
    for t in ri.MC_T:
        cnt = C.c_int64(-1)
        lib.check(L.bsn_robust_mc_count(dU.ptr, up.size, dL.ptr, lo.size, t, C.byref(cnt)))
        assert cnt.value == ri.mc_count_ref(up, lo, t), t
    for a, b in ri.MC_WINDOWS[kind]:
        want = ri.mc_window_ref(up, lo, a, b)
        cnt, buf = C.c_int64(-1), np.full(want.size, np.nan)
        lib.check(L.bsn_robust_mc_window(dU.ptr, up.size, dL.ptr, lo.size, a, b, want.size, _f(lib, buf), C.byref(cnt)))
        assert cnt.value == want.size and np.array_equal(np.sort(buf), want), (a, b)
        buf[:] = np.nan
        lib.check(L.bsn_robust_mc_window(dU.ptr, up.size, dL.ptr, lo.size, a, b, want.size - 1, _f(lib, buf), C.byref(cnt)))
        assert cnt.value == want.size and np.isnan(buf).all(), (a, b)        # over the cap: the count only, nothing written
    dU.free(); dL.free()


# ---- rolling mean -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,taps,offsets", ri.ROLL_CASES)
def test_rollmean_long_windows_short_groups(lib, m, taps, offsets):
    """k_rollmean at its limit of 4095 taps (32 KB of LDS) over groups of 300, 1, 4096 and 4603 values — two shorter than the
    window, one a single value — with one tap, with group edges at 255, 256 and 257 (below, on and above a workgroup edge), and
    without groups.  All terms are positive and added in order: numerator and denominator are each good to taps eps / 2, so
    the quotient to rtol = 2 taps eps with room."""
    L = lib.load()
    x, w = ri.roll_input(m), ri.rollmean_weights(taps)
    ref = ri.rollmean_ref(x, w, offsets)
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    got = np.full(m, np.nan)
    lib.check(L.bsn_robust_rollmean(_f(lib, x), m, _f(lib, w), taps, None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64)),
                                    0 if off is None else off.size - 1, _f(lib, got)))
    rel = np.abs(got.astype(LD) - ref) / ref
    print("m = %d, %d taps: max relative difference %.2e, bound %.2e" % (m, taps, float(rel.max()), 2 * taps * EPS))
    assert np.all(rel <= 2 * taps * EPS)


def test_rollmean_refusals(lib):
    L = lib.load()
    m = 1000
    x, out = ri.roll_input(m), np.empty(m)
    i64p = C.POINTER(C.c_int64)

    def call(taps, offsets):
        w = ri.rollmean_weights(taps)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        return L.bsn_robust_rollmean(_f(lib, x), m, _f(lib, w), taps, None if off is None else off.ctypes.data_as(i64p),
                                     0 if off is None else off.size - 1, _f(lib, out))

    _refused(lib, call(100, None), "an odd number of weights (at most 4095)")
    _refused(lib, call(4097, None), "an odd number of weights (at most 4095)")
    _refused(lib, call(101, (0, 400, 999)), "the groups do not cover the vector")
    _refused(lib, call(101, (1, 400, 1000)), "the groups do not cover the vector")
    _refused(lib, call(101, (0, 400, 400, 1000)), "empty group")
    assert call(101, (0, 400, 1000)) == 0


# ---- guards -----------------------------------------------------------------------------------------------------------------------

def test_guards(lib):
    """65 columns are refused where a thread holds a row of 64; ld < m is refused by every entry point that takes ld — before
    anything is launched"""
    L = lib.load()
    m = 300
    d = lib.DeviceArray(m, 65)
    v65, vm, nk = np.ones(65 * 65), np.ones(max(m, 65 * 32)), C.c_int64()

    def f(a):
        return _f(lib, a)

    at_most = "at most 64 columns"
    _refused(lib, L.bsn_robust_rotate(d.ptr, m, m, 65, f(v65)), at_most)
    _refused(lib, L.bsn_robust_pair_scales(d.ptr, m, m, 65, 4.5, 3.0, f(vm), f(vm)), at_most)
    _refused(lib, L.bsn_robust_dist_ogk(d.ptr, m, m, 65, 2, 1.5, 4.5, 3.0, f(vm), C.byref(nk)), at_most)
    ld = m - 1
    _refused(lib, L.bsn_robust_medians(d.ptr, m, ld, 3, None, f(vm)), "bsn_robust_medians: dimensions")
    _refused(lib, L.bsn_robust_scale_tau2(d.ptr, m, ld, 3, 4.5, 3.0, f(vm), f(vm)), "bsn_robust_scale_tau2: dimensions")
    _refused(lib, L.bsn_robust_pair_scales(d.ptr, m, ld, 3, 4.5, 3.0, f(vm), f(vm)), "bsn_robust_pair_scales: dimensions")
    _refused(lib, L.bsn_robust_scale_cols(d.ptr, m, ld, 3, f(vm)), "bsn_robust_scale_cols: dimensions")
    _refused(lib, L.bsn_robust_rotate(d.ptr, m, ld, 3, f(v65)), "bsn_robust_rotate: dimensions")
    _refused(lib, L.bsn_robust_wdist(d.ptr, m, ld, 3, f(vm), f(vm), f(vm)), "bsn_robust_wdist: dimensions")
    _refused(lib, L.bsn_robust_dist_ogk(d.ptr, m, ld, 3, 2, 1.5, 4.5, 3.0, f(vm), C.byref(nk)), "bsn_robust_dist_ogk: dimensions")
    d.free()
