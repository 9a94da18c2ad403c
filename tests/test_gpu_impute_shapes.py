"""The kernels of bigsnpr_amd/csrc/impute.hip where their loops take a second turn: the second 16-byte vector of a lane of
k_impute_2bit (and the Philox counter of its draws), the second turn of its row loop, more than one workgroup along the row in
both rewrite kernels, their variant stride, the second column chunk of the FBM bytes, the sample stride of k_impute_bytes,
and a dword whose sixteen fields are all missing.  The inputs are seeded (tests/helpers/impute_inputs.py);
tests/test_impute_shapes_cpu.py proves without a GPU, against the constants read from the source, that each shape crosses
the loop it is named for.

Every comparison is an equality with the CPU statement (tests/native/impute_ref.py): `check_edges`, as in
tests/test_gpu_impute.py — the FBM bytes, the number of variants without a call, the result image against the image
uploaded from its own bytes (pad bits included), and the products on both."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import impute_inputs as ii  # noqa: E402
import impute_ref as ref  # noqa: E402
from impute_inputs import METHODS, SEED, check_edges, column, impute, same_image  # noqa: E402


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def K():
    return ii.kernel_constants()


@pytest.fixture(scope="module")
def inputs(K):
    """name -> (matrix, intended number of variants without a call); built on first use, read-only"""
    made = {}

    def get(name):
        if name not in made:
            n, m = ii.shapes(K)[name]
            made[name] = ii.shape_matrix(n, m, K)
        return made[name]
    return get


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ii.SHAPE_NAMES)
def test_shapes_past_each_loop(ba, inputs, name, method):
    g, n_all = inputs(name)
    assert int((g == 3).all(0).sum()) == n_all
    check_edges(ba, g, method)
    if method == "mean2":
        # The pad bytes of the int8 image.  No accessor reads them, but the statistics over all samples (k_stats8) add up
        # the whole pitch and count on pad bytes of 0: a pad byte that took the table's entry for code 0 (index -100) would
        # lower the sum of its variant by 1.  In hundredths the sums are exact integers, taken here from the statement.
        want = ref.impute(g, method, seed=SEED)[0].astype(np.int64)
        kept = ~(g == 3).all(0)
        res = impute(ba, ba.FBM_code256(g), method, seed=SEED)
        st = ba.snp_colstats(res)
        assert np.array_equal(np.rint(100 * st["sumX"][kept]).astype(np.int64), np.where(g < 3, 100 * g.astype(np.int64), want - 7)[:, kept].sum(0))


def test_a_dword_with_all_sixteen_fields_missing(ba):
    """samples 16 .. 47 of variant 1 missing, every other genotype a call: fill_word_random draws sixteen times for one
    dword, field 15 (bits 30, 31) included"""
    g = ii.full_dword_matrix()
    j, (lo, hi) = ii.FULL_COLUMN, ii.FULL_MISSING
    col = g[:, j]
    af = ref.rule_af(int((col == 1).sum()), int((col == 2).sum()), int((col < 3).sum()))
    draws = np.array([ref.draw(SEED, i, j, af) for i in range(lo, hi)])
    for method in ("random", "mode"):
        check_edges(ba, g, method)
        res = impute(ba, ba.FBM_code256(g), method, seed=SEED, return_bytes=True)
        want, val, _ = ref.impute(g, method, seed=SEED)
        fill = draws if method == "random" else np.full(hi - lo, val[j])
        assert np.array_equal(res.bytes[lo:hi, j], 4 + fill)                 # the FBM bytes, position by position
        got = column(ba, res, j)                                             # the image, through the accessor
        assert np.array_equal(got[lo:hi], fill) and np.array_equal(got, np.where(col == 3, want[:, j] - 4, col))
        same_image(ba, res)
