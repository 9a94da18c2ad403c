"""The inputs of tests/test_gpu_dosage_slices.py (tests/helpers/dosage_inputs.py) without a GPU: each panel is past the size
at which one int32 accumulator stops being enough, in a way a wrong kernel cannot survive — sums that pass 2^31 over the
whole row and stay below it per slice, a second slice that moves nearly every correlation, thresholds far from every
reference value, and a vector whose digits do not cancel.  Every sum here is a float64 matmul of integers below 2^53."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import dosage_inputs as di  # noqa: E402

WINDOW = 40                  # kb, the windows of the device test
THRESHOLDS = (0.1, 0.2)      # thr_r2 of its snp_cor and snp_clumping calls
ALPHA = 0.05


@pytest.fixture(scope="module")
def panel():
    return di.slice_panel()


@pytest.fixture(scope="module")
def sums(panel):
    return di.PairSums(panel[0])


def test_tables():
    assert di.GRID255.size == 256 and np.isnan(di.GRID255[255])
    np.testing.assert_array_equal(di.GRID255[:255], np.arange(255) - 127.0)
    k = np.arange(-127, 128).astype(np.int8)[:, None]
    np.testing.assert_array_equal(di.GRID255[di.grid255_bytes(k)[:, 0]], k[:, 0])          # the value IS the grid index
    d = di.dosage_indices(k)
    assert d.min() == -100 and d.max() == 100
    np.testing.assert_allclose(di.CODE_DOSAGE[di.dosage_bytes(d)[:, 0]], 1.0 + 0.01 * d[:, 0], rtol=0, atol=1e-15)
    miss = np.zeros(k.shape, dtype=bool)
    miss[5] = True
    assert np.isnan(di.GRID255[di.grid255_bytes(k, miss)[5, 0]]) and np.isnan(di.CODE_DOSAGE[di.dosage_bytes(d, miss)[5, 0]])
    # the size argument of bigsnpr_amd/csrc/byte_plan.hpp
    assert di.TERM_MAX * di.SLICE < 2 ** 31 <= di.TERM_MAX * (di.SLAB_TERMS + 1) and di.SLAB_TERMS == 132104


def test_slice_panel_shape(panel):
    k, pos = panel
    assert k.shape == (di.SLICE_N, di.SLICE_M) == (135300, 192) and k.dtype == np.int8
    assert di.pitch_of(di.SLICE_N) == 135424 and di.SLICE < di.pitch_of(di.SLICE_N) < 2 * di.SLICE   # two slices, ragged
    assert np.abs(k.astype(np.int16)).max() == 127 and k.min() == -127
    assert np.all(np.diff(pos) > 0)
    a, b = (k[:, j].astype(np.int64) for j in di.TWINS)
    assert set(np.unique(a)) == {-127, 127} and (a == -127).sum() == di.SLICE_N // 100
    assert (a != b).sum() == 50
    for v in (a == -127, a != b):
        assert v[:di.SLICE].any() and v[di.SLICE:].any()                                  # spread over both slices


def test_the_twins_pass_2_31_only_over_the_whole_row(panel, sums):
    k = panel[0]
    a, b = (k[:, j].astype(np.int64) for j in di.TWINS)
    total, first = int((a * b).sum()), int((a[:di.SLICE] * b[:di.SLICE]).sum())
    assert (total, first) == (2180640800, 2112511904)
    assert total == sums.xy[di.TWINS[0], di.TWINS[1]]
    assert first < 2 ** 31 < total and total - first < 2 ** 31
    # ... and so does a twin's sum of squares, the largest entry of the cross-product matrix
    assert sums.xy[0, 0] == np.abs(sums.xy).max() == 127 ** 2 * di.SLICE_N == 2182253700 > 2 ** 31 > 127 ** 2 * di.SLICE


def test_the_second_slice_moves_nearly_every_correlation(panel, sums):
    k, pos = panel
    r = sums.r()[0]
    r_head = di.PairSums(k[:di.SLICE]).r()[0]
    r_twice = di.PairSums(np.concatenate([k, k[di.SLICE:]])).r()[0]     # the second slice booked twice
    pairs = di.window_pairs(pos, WINDOW)
    j0 = np.concatenate([np.full(js.size, t) for t, js in enumerate(pairs)])
    j = np.concatenate(pairs)
    assert j.size > 4000
    for other in (r_head, r_twice):
        moved = np.abs((r - other)[j0, j]) > 1e-6
        assert moved.mean() > 0.9, moved.mean()


@pytest.mark.parametrize("rows", ["all", "subset"])
def test_no_reference_value_sits_on_a_threshold(panel, sums, rows):
    from oracle import oracle as orc
    k, pos = panel
    s = sums if rows == "all" else di.PairSums(k, rows=di.slice_rows())
    r, r2, _ = s.r()
    pairs = di.window_pairs(pos, WINDOW)
    j0 = np.concatenate([np.full(js.size, t) for t, js in enumerate(pairs)])
    j = np.concatenate(pairs)
    for thr in THRESHOLDS:
        assert np.abs(r2[j0, j] - thr).min() > 1e-6
        assert 0.05 < (r2[j0, j] > thr).mean() < 0.95           # and the threshold cuts through the band
    t = orc.cor_thresholds(s.n, ALPHA)[s.n - 1]
    assert 0 < t < 0.01 and np.abs(np.abs(r[j0, j]) - t).min() > 1e-7
    # the CODE_DOSAGE re-expression (clipped to +-100) for the clumping threshold
    rd2 = di.PairSums(di.dosage_indices(k), rows=None if rows == "all" else di.slice_rows()).r()[1]
    assert np.abs(rd2[np.tril_indices(di.SLICE_M, -1)] - 0.2).min() > 1e-6


def test_missing_version(panel):
    k, pos = panel
    miss = di.slice_missing()
    assert 0.025 < miss.mean() < 0.04
    assert miss[:, 11].mean() > 0.5 and miss[:, 40].sum() == 2 and miss[3].all() and miss[di.SLICE + 77].all()
    assert miss[:di.SLICE].any() and miss[di.SLICE:].any()
    s = di.PairSums(k, miss)
    # pairwise complete: the counts differ from pair to pair, and the sums of the first variant depend on the second
    assert np.unique(s.nona).size > 500 and np.all(s.nona <= di.SLICE_N - 2)
    assert np.all(s.nona == s.nona.T) and np.all(s.xy == s.xy.T) and not np.all(s.xs == s.xs[:, :1])
    # the sums from a plain loop over one pair
    x, y = k[:, 17].astype(np.int64), k[:, 5].astype(np.int64)
    both = ~miss[:, 17] & ~miss[:, 5]
    assert (s.xy[17, 5], s.nona[17, 5], s.xs[17, 5], s.xx[17, 5], s.xs[5, 17], s.xx[5, 17]) == \
        ((x * y)[both].sum(), both.sum(), x[both].sum(), (x * x)[both].sum(), y[both].sum(), (y * y)[both].sum())
    r = s.r()[0]
    assert np.isfinite(r[np.tril_indices(di.SLICE_M, -1)]).all()


def test_references_agree_with_a_direct_evaluation(panel):
    """cor_reference / ld_scores_reference on a corner of the panel small enough for np.corrcoef"""
    k, pos = panel
    kk, pp = k[:3000, :30], pos[:30]
    s = di.PairSums(kk)
    R = np.corrcoef(kk.astype(np.float64), rowvar=False)
    thr = np.full(3000, np.sqrt(0.1))
    i, p, x, margin = di.cor_reference(s, pp, WINDOW, thr)
    assert margin > 0 and p[0] == 0 and p[-1] == i.size == x.size
    for j0 in range(30):
        js = np.array([j for j in range(j0) if pp[j] >= pp[j0] - WINDOW * 1000.0 and R[j0, j] ** 2 > 0.1] + [j0])
        np.testing.assert_array_equal(i[p[j0]:p[j0 + 1]], js)
        np.testing.assert_allclose(x[p[j0]:p[j0 + 1]], R[j0, js], rtol=0, atol=1e-12)
    ld = np.ones(30)
    for j0 in range(30):
        for j in range(j0):
            if pp[j] >= pp[j0] - WINDOW * 1000.0:
                ld[j0] += R[j0, j] ** 2
                ld[j] += R[j0, j] ** 2
    np.testing.assert_allclose(di.ld_scores_reference(s, pp, WINDOW), ld, rtol=1e-12)


def test_overflow_panel():
    k = di.overflow_panel()
    assert k.shape == (di.OVER_N, di.OVER_M) == (132352, 130) and di.pitch_of(di.OVER_N) == di.OVER_N
    assert di.OVER_N == (di.SLAB_TERMS // 256 + 1) * 256                  # the smallest pitch above 132 104
    assert di.OVER_M % 16 != 0 and di.OVER_M // 16 == 8
    assert np.all(k[:, 0] == 127) and np.all(k[:, 1] == -127) and set(np.unique(k[:, 2])) == {-127, 127}
    assert k[:, 2].astype(np.int64).sum() == 0 and k[:, 3:].min() == -127 and k[:, 3:].max() == 127
    # y = 32128 at seven digits: scale 2^40 and the digits of the issue, the same for every sample
    qs, d = di.quant_digits(np.full(di.OVER_N, di.OVER_Y), 7)
    assert qs == 2.0 ** 40
    assert np.all(d == np.array([0, 0, 0, 0, 0, -128, 126]))
    # the digits recompose to y qscale, whatever the vector
    y = np.random.default_rng(0).normal(size=1000)
    for S in (2, 4, 7):
        q, dd = di.quant_digits(y, S)
        assert dd.min() >= -128 and dd.max() <= 127
        np.testing.assert_array_equal((dd * 256 ** np.arange(S)).sum(1), np.rint(y * q).astype(np.int64))
    # one int32 over the whole sample range wraps in the -128 column of variant 0 (and of 1, the other way) ...
    col = d[:, 5].astype(np.float64) @ k.astype(np.float64)
    assert col[0] == -128 * 127 * di.OVER_N == -2151514112 and col[0] < -2 ** 31 and col[1] > 2 ** 31 - 1
    assert abs(col[2]) == 0 and np.abs(col[3:]).max() < 2 ** 31
    # ... and not per slice
    assert np.abs(d[:di.SLICE, 5].astype(np.float64) @ k[:di.SLICE].astype(np.float64)).max() < 2 ** 31
    # the wrapped sum is wrong by 2^32 * 256^5 / 2^40 = 2^32 in z: six orders above the test's tolerance
    ref = di.cprod_reference(k, np.full(di.OVER_N, di.OVER_Y))
    assert ref[0] == 127 * di.OVER_Y * di.OVER_N
    assert 2.0 ** 32 > 1e6 * 1e-9 * np.abs(ref).max()
