"""snp_fst and snp_MAX3 without a GPU: the CPU statement (tests/native/popstat_ref.cpp over popstat_step.hpp, the header
the kernels are compiled from) against the nine published MAX3 statistics of Zheng et al. 2012 (the reference's own test,
tests/testthat/test-4-MAX3.R), against an independent numpy restatement of R/Fst.R and R/MAX3.R on random count tables
and on the special cases, the order of the `overall` sums against math.fsum, and the reference's example populations."""
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

import popstat_ref as ref  # noqa: E402
from impute_ref import read_bed_bytes  # noqa: E402


# ---- the direct definitions -----------------------------------------------------------------------------------------------
def numpy_fst(af, N, min_maf=0.0):
    """R/Fst.R:57-84 on arrays (r, m): (a, a + b + c, keep)"""
    af, N = np.asarray(af, dtype=np.float64), np.asarray(N, dtype=np.float64)
    r = af.shape[0]
    with np.errstate(all="ignore"):
        n_sum = N.sum(axis=0)
        n_bar = n_sum / r
        n_c = (n_sum - (N ** 2).sum(axis=0) / n_sum) / (r - 1)
        p_bar = (af * N).sum(axis=0) / n_sum
        s2 = ((af - p_bar) ** 2 * N).sum(axis=0) / n_bar / (r - 1)
        h_bar = (2 * af * (1 - af) * N).sum(axis=0) / n_sum
        a = n_bar / n_c * (s2 - 1 / (n_bar - 1) * (p_bar * (1 - p_bar) - (r - 1) / r * s2 - h_bar / 4))
        b = n_bar / (n_bar - 1) * (p_bar * (1 - p_bar) - (r - 1) / r * s2 - (2 * n_bar - 1) / (4 * n_bar) * h_bar)
        c = h_bar / 2
        keep = (p_bar > min_maf) & (p_bar < 1 - min_maf)
        abc = a + b + c
    return a, abc, keep


def numpy_max3(cases, controls, val=(0, 0.5, 1)):
    """R/MAX3.R:3-28,95-103 on 3 x m count tables"""
    rj, sj = np.asarray(cases, dtype=np.float64), np.asarray(controls, dtype=np.float64)
    with np.errstate(all="ignore"):
        r, s = rj.sum(axis=0), sj.sum(axis=0)
        n = r + s
        phi = r / n
        num = rj * (1 - phi) - sj * phi
        pj = (rj + sj) / n
        coef = n * phi * (1 - phi)
        stats = []
        for x in np.atleast_1d(val):
            x2 = np.array([0.0, x, 1.0])[:, None]
            deno = (x2 ** 2 * pj).sum(axis=0) - (x2 * pj).sum(axis=0) ** 2
            stats.append((x2 * num).sum(axis=0) / np.sqrt(coef * deno))
        z = np.array(stats)
    z[np.isnan(z)] = 0.0
    return (z ** 2).max(axis=0)


def close(a, b, rtol=1e-12):
    """equal to a relative 1e-12 (numpy may associate the sums differently), NaN == NaN, inf == inf"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.allclose(a, b, rtol=rtol, atol=0.0, equal_nan=True)


def same_fst(t, a, abc, keep, tol_abs=0.0):
    """terms of the kept variants, and which variants are kept (NaN and `not kept` are the same answer)"""
    assert np.array_equal(t["keep"], keep)
    assert close(t["a"][keep], a[keep]) and close(t["abc"][keep], abc[keep])
    assert np.isnan(t["fst"][~keep]).all()
    assert close(t["fst"][keep], a[keep] / abc[keep], rtol=1e-11)   # (a quotient of two sums each good to 1e-12)


def random_tables(rng, r, m, nmax=400):
    """counts (r, 4, m) of 0 / 1 / 2 / NA for r groups of random sizes"""
    out = np.empty((r, 4, m), dtype=np.int64)
    sizes = rng.integers(2, nmax, size=r)
    for p in range(r):
        f = rng.uniform(0.02, 0.98, size=m)
        prob = np.stack([(1 - f) ** 2 * 0.97, 2 * f * (1 - f) * 0.97, f ** 2 * 0.97, np.full(m, 0.03)], axis=1)
        out[p] = np.array([rng.multinomial(sizes[p], pr) for pr in prob]).T
    return out, sizes


def maf(counts_r4m):
    c = np.asarray(counts_r4m, dtype=np.int64)
    N = c[:, 0] + c[:, 1] + c[:, 2]
    with np.errstate(all="ignore"):
        return (c[:, 1] + 2 * c[:, 2]) / (2.0 * N), N.astype(np.float64)


# ---- MAX3 against the published table -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zheng(golden_dir):
    with open(os.path.join(golden_dir, "max3_zheng2012.json")) as f:
        z = json.load(f)
    cases, controls = np.array(z["cases"]).T, np.array(z["controls"]).T
    assert cases.shape == controls.shape == (3, 9) and len(z["sqrt_score"]) == 9
    return cases, controls, np.array(z["sqrt_score"])


def test_max3_reproduces_the_published_statistics(zheng):
    cases, controls, want = zheng
    got = np.sqrt(ref.max3(cases, controls))
    assert np.array_equal(np.round(got, 3), want), got
    assert np.array_equal(np.round(np.sqrt(numpy_max3(cases, controls)), 3), want)
    # (no value near a rounding boundary of the third decimal)
    assert (np.abs(got * 1000 - np.floor(got * 1000) - 0.5) > 0.02).all()


# ---- the statement against numpy -------------------------------------------------------------------------------------------
def test_af_is_bed_maf():
    rng = np.random.default_rng(0)
    for c1, c2, N in rng.integers(0, 5000, size=(200, 3)):
        N = max(N, (c1 + c2))
        if N == 0:
            assert math.isnan(ref.af(c1, c2, N))
        else:
            assert ref.af(c1, c2, N) == (c1 + 2 * c2) / (2.0 * N)
    assert math.isnan(ref.af(0, 0, 0))


@pytest.mark.parametrize("r", [2, 3, 5, 26])
def test_fst_terms_against_numpy(r):
    rng = np.random.default_rng(10 + r)
    counts, _ = random_tables(rng, r, 300)
    af, N = maf(counts)
    for min_maf in (0.0, 0.05):
        same_fst(ref.fst(af, N, min_maf), *numpy_fst(af, N, min_maf))


@pytest.mark.parametrize("val", [(0, 0.5, 1), (0.5,), (0, 1), tuple(np.linspace(0, 1, 33))])
def test_max3_against_numpy(val):
    rng = np.random.default_rng(21)
    counts, _ = random_tables(rng, 2, 400)
    got, want = ref.max3(counts[1, :3], counts[0, :3], val), numpy_max3(counts[1, :3], counts[0, :3], val)
    assert np.isfinite(got).all() and (got >= 0).all() and close(got, want)


# ---- the special cases -------------------------------------------------------------------------------------------------------
def test_fst_special_cases():
    #                 variant: ordinary  monomorphic  empty pop.  all NA in g1   rare (p_bar < 0.05)  fixed in both at 1
    counts = np.array([[[50, 100, 0, 100, 95, 0], [30, 0, 0, 0, 5, 0], [20, 0, 0, 0, 0, 100], [0, 0, 100, 0, 0, 0]],
                       [[20, 80, 40, 0, 78, 0], [40, 0, 30, 0, 2, 0], [20, 0, 10, 0, 0, 80], [0, 0, 0, 80, 0, 0]]])
    af, N = maf(counts)
    assert np.isnan(af[0, 2]) and N[0, 2] == 0 and np.isnan(af[1, 3]) and N[1, 3] == 0
    t = ref.fst(af, N, 0.0)
    same_fst(t, *numpy_fst(af, N, 0.0))
    assert t["keep"].tolist() == [True, False, False, False, True, False]
    t = ref.fst(af, N, 0.05)
    same_fst(t, *numpy_fst(af, N, 0.05))
    assert t["keep"].tolist() == [True, False, False, False, False, False]
    # the overall value takes the kept variants only: the NaN terms of the others do not reach it
    assert t["overall"][0] == t["fst"][0] and np.isfinite(t["overall"]).all()


def test_fst_n_bar_of_one():
    """two populations of one sample each: n_bar - 1 = 0; whatever the reference's expressions give, so does the statement"""
    af, N = np.array([[0.5, 0.0], [0.0, 1.0]]), np.array([[1.0, 1.0], [1.0, 1.0]])
    t, (a, abc, keep) = ref.fst(af, N, 0.0), numpy_fst(af, N, 0.0)
    assert np.array_equal(t["keep"], keep) and keep.all()
    assert close(t["a"], a) and close(t["abc"], abc)
    assert not np.isfinite(t["a"]).any()   # (1 / 0 enters both terms)


def test_max3_special_cases():
    # cases only: phi = 1, every statistic is 0 / 0 -> 0; controls only likewise; nobody at all; a monomorphic variant
    cases = np.array([[10, 0, 0, 40], [20, 0, 0, 0], [5, 0, 0, 0]])
    controls = np.array([[0, 12, 0, 50], [0, 7, 0, 0], [0, 3, 0, 0]])
    got = ref.max3(cases, controls)
    assert got.tolist() == [0.0, 0.0, 0.0, 0.0]
    assert numpy_max3(cases, controls).tolist() == [0.0, 0.0, 0.0, 0.0]


# ---- the order of the overall sums -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 255, 256, 257, 1000])
def test_overall_sums_against_fsum(m):
    rng = np.random.default_rng(m)
    counts, _ = random_tables(rng, 3, m)
    counts[:, :, ::7] = counts[:, :, ::7].sum(axis=1, keepdims=True) * np.array([1, 0, 0, 0])[None, :, None]   # monomorphic
    af, N = maf(counts)
    t = ref.fst(af, N, 0.05)
    keep = t["keep"]
    assert (m == 1) or (0 < keep.sum() < m)
    for got, terms in ((t["overall"][1], t["a"][keep]), (t["overall"][2], t["abc"][keep])):
        exact = math.fsum(terms)
        bound = (m - 1) * 2.0 ** -53 * math.fsum(np.abs(terms))
        print("m = %d: |sum - fsum| = %.3e, bound %.3e" % (m, abs(got - exact), bound))
        assert abs(got - exact) <= bound
    if keep.any():
        assert t["overall"][0] == t["overall"][1] / t["overall"][2]
    # the reduction alone, on terms of mixed sign
    x = rng.normal(size=m) * 10.0 ** rng.integers(-3, 4, size=m)
    assert abs(ref.block_sum(x) - math.fsum(x)) <= (m - 1) * 2.0 ** -53 * math.fsum(np.abs(x))


# ---- the reference's example ----------------------------------------------------------------------------------------------------
def test_example_bed_anchor(golden_dir):
    """R/Fst.R:35-45 and tests/testthat/test-9-Fst.R: populations of 143, 167 and 207 rows of example.bed"""
    G = read_bed_bytes(os.path.join(golden_dir, "example.bed"), 517, 4542)
    pop = np.repeat([0, 1, 2], [143, 167, 207])
    counts = np.array([[(G[pop == p] == c).sum(axis=0) for c in range(4)] for p in range(3)])
    af, N = maf(counts)
    for p in range(3):   # the frequencies as the header forms them are bed_MAF's
        a2, n2 = ref.maf_from_counts(counts[p], int((pop == p).sum()))
        assert np.array_equal(a2, af[p]) and np.array_equal(n2, N[p])
    t = ref.fst(af, N, 0.0)
    assert t["keep"].all() and t["keep"].size == 4542
    assert 0.0236 <= t["overall"][0] <= 0.0238, t["overall"]
    same_fst(t, *numpy_fst(af, N, 0.0))
    a, abc, keep = numpy_fst(af, N, 0.0)
    assert abs(a.sum() / abc.sum() - t["overall"][0]) <= 1e-12
    for pair in ((0, 1), (0, 2), (2, 1)):
        tp = ref.fst(af[list(pair)], N[list(pair)], 0.0)
        a, abc, keep = numpy_fst(af[list(pair)], N[list(pair)], 0.0)
        assert np.array_equal(tp["keep"], keep) and abs(a[keep].sum() / abc[keep].sum() - tp["overall"][0]) <= 1e-12
