"""snp_fastImputeSimple without a GPU: the CPU statement (tests/native/impute_ref.cpp over impute_step.hpp, the header the
kernels are compiled from) against a direct numpy definition on example-missing.bed, the reference's own expectations
(tests/testthat/test-3-fastImpute.R:111-142), the rounding cases where the double operations and the exact rational part
ways, the mode ties, the statistics and independence of `random`, the header under a sanitizer as a stand-alone
program, and the argument errors of the host mirror."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

import impute_ref as ref  # noqa: E402

METHODS = ("zero", "mode", "mean0", "mean2", "random")
# `random`: seeds tried on the CPU statement with impute_ref.chi_square_column(); p-values of the goodness of fit
# 0.53 / 0.44 / 0.64 — far above the 1e-4 the reference asks for (test-3-fastImpute.R:138).  The device is bit-equal
# to the statement, so tests/test_gpu_impute.py runs the same check with impute_ref.SEED.
SEED, OTHER_SEEDS = ref.SEED, (1, 987654321)
TAG = 0x494D5053


# ---- the direct definition ----------------------------------------------------------------------------------------------
def philox4x32_10(c, k):
    """Salmon et al. 2011 on arrays: c = four uint32 arrays, k = two uint32 scalars"""
    c = [np.asarray(x, dtype=np.uint64) for x in c]
    k0, k1 = int(k[0]), int(k[1])
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        a, b = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(b >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), b & M, (a >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), a & M]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def unit_open(a, b):
    n = (a << np.uint64(20)) | (b >> np.uint64(12))
    return (2.0 * n.astype(np.float64) + 1.0) * 2.0 ** -53


def numpy_impute(G, method, seed=0):
    """snp_fastImputeSimple on FBM bytes (n x m, 3 = missing), written from the issue's table: (bytes, n_all_missing)"""
    G = np.asarray(G, dtype=np.uint8)
    n, m = G.shape
    out, n_all = G.copy(), 0
    for j in range(m):
        col = G[:, j]
        na = np.flatnonzero(col > 2)
        c1, c2 = int((col == 1).sum()), int((col == 2).sum())
        c = n - na.size
        c0 = c - c1 - c2
        n_all += c == 0
        if method == "zero":
            continue
        if method == "mode":
            v = 0
            if c1 > c0:
                v = 1
            if v == 0 and c2 > c0:
                v = 2
            if v == 1 and c2 > c1:
                v = 2
            out[na, j] = 4 + v
        elif c == 0:
            continue
        elif method == "mean0":
            out[na, j] = 4 + int(np.rint((c1 + 2.0 * c2) / c))
        elif method == "mean2":
            out[na, j] = 7 + int(np.rint(100 * ((c1 + 2.0 * c2) / c)))
        else:
            af = (0.5 * c1 + c2) / c
            z = np.zeros(na.size, dtype=np.uint64)
            o = philox4x32_10([na.astype(np.uint64), z + np.uint64(j), z + np.uint64(TAG), z],
                              (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
            out[na, j] = 4 + (unit_open(o[0], o[1]) < af).astype(np.uint8) + (unit_open(o[2], o[3]) < af).astype(np.uint8)
    return out, int(n_all)


@pytest.fixture(scope="module")
def G(golden_dir):
    return ref.read_bed_bytes(os.path.join(golden_dir, "example-missing.bed"), 200, 500)


def test_example_data_is_what_the_issue_says(G):
    na = G == 3
    assert G.shape == (200, 500) and na.sum() == 2788 and (na.sum(0) > 0).sum() == 367 and na.sum(0).max() == 53
    assert [(G[:, 399] == k).sum() for k in range(4)] == [42, 112, 44, 2] and list(np.flatnonzero(na[:, 399])) == [17, 71]
    assert [(G[:, 0] == k).sum() for k in range(3)] == [183, 8, 0] and na[3, 0] and na[11, 0]


@pytest.mark.parametrize("method", METHODS)
def test_statement_against_the_numpy_definition(G, method):
    got, val, n_all = ref.impute(G, method, seed=SEED)
    want, want_all = numpy_impute(G, method, seed=SEED)
    assert np.array_equal(got, want) and n_all == want_all == 0
    assert np.array_equal(got[G != 3], G[G != 3])                      # a call is never touched
    lo, hi = {"zero": (3, 3), "mean2": (7, 207)}.get(method, (4, 6))
    assert got[G == 3].min() >= lo and got[G == 3].max() <= hi
    assert np.array_equal(ref.impute(G, method, seed=SEED, nthreads=4)[0], got)   # (test-3-fastImpute.R:140-141)


def test_the_references_own_expectations(G):
    """tests/testthat/test-3-fastImpute.R:117-130, 1-based there"""
    assert list(G[[17, 71], 399]) == [3, 3]                                 # the source decodes them as NA
    assert list(ref.impute(G, "zero")[0][[17, 71], 399]) == [3, 3]          # byte 3, which the new table decodes as 0
    assert list(ref.impute(G, "mean0")[0][[17, 71], 399]) == [5, 5]         # 1
    assert list(ref.impute(G, "mean2")[0][[17, 71], 399]) == [108, 108]     # 1.01
    mode = ref.impute(G, "mode")[0]
    assert list(mode[[3, 11], 0]) == [4, 4] and list(mode[[17, 71], 399]) == [5, 5]
    assert list(G[[17, 71], 399]) == [3, 3]                                 # and still does


def _counts_for(c, s):
    c2 = max(0, s - c)
    return s - 2 * c2, c2


@pytest.mark.parametrize("c,s,want", [(40, 23, 57), (40, 49, 123), (40, 51, 127), (8, 1, 12), (8, 5, 62)])
def test_mean2_rounds_the_double_operations(c, s, want):
    """r = nearbyint(100 * (s / c)) in fp64, ties to even — not the exact rational 100 s / c, not half up"""
    c1, c2 = _counts_for(c, s)
    assert ref.rule_val("mean2", c1, c2, c) == want
    col = np.array([1] * c1 + [2] * c2 + [0] * (c - c1 - c2) + [3, 3], dtype=np.uint8)
    out = ref.impute(col, "mean2")[0]
    assert list(out[-2:, 0]) == [7 + want] * 2
    assert np.array_equal(out, numpy_impute(col[:, None], "mean2")[0])


@pytest.mark.parametrize("c,s,want", [(2, 1, 0), (2, 3, 2)])
def test_mean0_ties_to_even(c, s, want):
    c1, c2 = _counts_for(c, s)
    assert ref.rule_val("mean0", c1, c2, c) == want
    col = np.array([3] + [1] * c1 + [2] * c2 + [0] * (c - c1 - c2), dtype=np.uint8)
    assert ref.impute(col, "mean0")[0][0, 0] == 4 + want


@pytest.mark.parametrize("c0,c1,c2,want", [(4, 4, 2, 0), (2, 4, 4, 1), (4, 2, 4, 0), (3, 3, 3, 0),
                                           (5, 3, 1, 0), (3, 5, 1, 1), (1, 3, 5, 2), (3, 1, 5, 2)])
def test_mode_ties_go_to_the_smaller_call(c0, c1, c2, want):
    assert ref.rule_val("mode", c1, c2, c0 + c1 + c2) == want
    col = np.array([3] + [0] * c0 + [1] * c1 + [2] * c2 + [3], dtype=np.uint8)
    out = ref.impute(col, "mode")[0]
    assert list(out[[0, -1], 0]) == [4 + want] * 2
    assert np.array_equal(out, numpy_impute(col[:, None], "mode")[0])


def test_a_variant_without_any_call():
    """mode gives 0 like the reference; mean0 / mean2 / random leave it missing (the reference casts a NaN to a byte)"""
    Gm = np.array([[3, 0, 3], [3, 1, 3], [3, 3, 3]], dtype=np.uint8)
    for method in METHODS:
        out, val, n_all = ref.impute(Gm, method, seed=5)
        assert n_all == 2
        want = {"zero": 3, "mode": 4}.get(method, 3)
        assert (out[:, [0, 2]] == want).all() and list(val[[0, 2]]) == [0 if method in ("zero", "mode") else -1] * 2
        assert np.array_equal(out, numpy_impute(Gm, method, seed=5)[0])


@pytest.mark.parametrize("seed", (SEED,) + OTHER_SEEDS)
def test_random_follows_the_allele_frequency(seed):
    col = ref.chi_square_column()
    assert (col == 3).sum() >= 1000
    out = ref.impute(col, "random", seed=seed)[0][:, 0]
    pv = ref.chi_square_pvalue(col, out)
    print("seed", seed, "p-value", pv)
    assert pv > 1e-4
    assert np.array_equal(out, numpy_impute(col[:, None], "random", seed=seed)[0][:, 0])


def test_random_draws_differ_between_variants_and_seeds():
    col = ref.chi_square_column()
    G2 = np.asfortranarray(np.stack([col, col], axis=1))   # the same counts, the same missing rows
    out = ref.impute(G2, "random", seed=SEED)[0]
    na = col == 3
    assert not np.array_equal(out[na, 0], out[na, 1])
    assert 0.3 < (out[na, 0] == out[na, 1]).mean() < 0.7   # independent draws agree 0.45 of the time at p = 0.3
    assert np.array_equal(ref.impute(G2, "random", seed=SEED)[0], out)
    assert not np.array_equal(ref.impute(G2, "random", seed=SEED + 1)[0], out)
    assert ref.draw(SEED, 5, 9, 0.3) == ref.draw(SEED, 5, 9, 0.3)


def test_header_under_a_sanitizer(tmp_path):
    """rules, draw, c == 0 and n % 4 != 0 as a stand-alone program built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "impute_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-ffp-contract=off", "-std=c++17",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "bigsnpr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "impute_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks held" in out.stdout


def test_argument_errors_need_no_gpu():
    import bigsnpr_amd as ba
    Gna = ba.FBM_code256.__new__(ba.FBM_code256)   # the checks come before the image is looked at
    Gna.code256, Gna._bed = ba.CODE_IMPUTE_PRED, None
    with pytest.raises(ValueError, match="identical.*CODE_012.* is not TRUE"):
        ba.snp_fastImputeSimple(Gna)
    Gna.code256 = ba.CODE_012.copy()
    with pytest.raises(ValueError, match="should be one of"):
        ba.snp_fastImputeSimple(Gna, "mean")
    with pytest.raises(TypeError, match="not of class 'FBM.code256'"):
        ba.snp_fastImputeSimple(np.zeros((3, 3), dtype=np.uint8))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(Warning, match="deprecated"):
            ba.snp_fastImputeSimple(Gna, "zero")
