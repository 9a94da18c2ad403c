"""k_prodT's one-dimensional grid (bigsnpr_amd/csrc/prod_plan.hpp: prodt_slab): the sample blocks that fill whole rounds of
the CUs run in few long workgroups, the blocks beyond the last whole round in many short ones, and k_prod_final adds as many
slabs as the row has.  A shape of a few thousand samples never fills a round of the device's CUs, so every case runs with
BSN_PLAN_CUS=4 (the CU count the planner assumes) and pins, through the planner on the CPU, the geometry it is about.  The sums
are the integers of k_prod on the variant-major image (BSN_NO_SMAJ=1): every product and a whole solve are compared bit for
bit with that path, as tests/test_gpu_smaj.py compares."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

M = 6661   # 14 chunks of 512 variants (13 behind variant 512): the remainder's 5 slabs of 3 chunks end in a short one
# name -> samples, first variant, (wgx, wgx_whole) with 4 CUs
SHAPES = {
    "two rounds and two blocks": (4645, 0, (10, 8)),      # the last block has 37 rows
    "two rounds": (4096, 0, (8, 8)),                      # no remainder
    "less than a round": (1500, 0, (3, 0)),               # the geometry as it was
    "from variant 512": (4645, 512, (10, 8)),
}
# name -> slices, environment, missing genotypes per 65 536, k_prodT<NB, HASQ, ., ., ., ., NASKIP, SPARSE> of the launch
PANELS = {
    "16 x 24 bits sparse": (3, {"BSN_NA_SKIP": "0"}, 655, (3, True, False, True)),
    "16 x 24 bits dense": (3, {"BSN_NA_SKIP": "0", "BSN_NO_SPARSE_PROD": "1"}, 655, (3, True, False, False)),
    "16 x 16 bits": (2, {"BSN_NA_SKIP": "0"}, 655, (2, True, False, False)),
    "complete data": (3, {}, 0, (3, False, False, False)),
    "skipping kernels 24 bits": (3, {"BSN_NA_SKIP": "1"}, 655, (3, True, True, False)),
    "skipping kernels 16 bits": (2, {"BSN_NA_SKIP": "1"}, 655, (2, True, True, False)),
}


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def images(ba):
    """one image per (samples, missing rate), with its code counts (an operator learns from them that the data is complete)
    and its sample-major copy"""
    made = {}

    def get(n, na16):
        if (n, na16) not in made:
            gb = ba.bed.synthetic(n, M, seed=n + na16, na16=na16)
            ba.bed_counts(gb)
            assert gb.sample_major()
            made[(n, na16)] = gb
        return made[(n, na16)]
    yield get
    for gb in made.values():
        gb.close()


def template_args(name):
    assert "k_prodT<" in name, name
    a = [t.strip() for t in name.split("<", 1)[1].rstrip("> ").split(",")]
    return int(a[0]), a[1] == "true", a[6] == "true", a[7] == "true"


def planned(n, m, col0, S):
    import prodt_grid_ref as pg
    f = dict(bits=2, n=n, m=m, pitch=(n + 511) // 512 * 128, col0=col0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1,
             no_sparse=0, nvec=16, S=S, ncu=4, segmented=0)
    assert pg.check(**f) == 0
    return pg.plan(**f)


@pytest.mark.parametrize("panel", list(PANELS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_product_is_bit_identical_to_k_prod(ba, images, monkeypatch, shape, panel):
    from bigsnpr_amd import _lib
    sync = _lib.load().bsn_device_sync
    n, col0, (wgx, wgx_whole) = SHAPES[shape]
    S, env, na16, want = PANELS[panel]
    m = M - col0
    # the geometry this case is about (the planner with 4 CUs; the default slab count of the whole rounds is 1 .. 3)
    p = planned(n, m, col0, S)
    assert (p["smaj"], p["wgx"], p["wgx_whole"]) == (1, wgx, wgx_whole), p
    if wgx_whole:
        assert 1 <= p["ky_whole"] <= 3 and p["ky"] > p["ky_whole"] and p["ky"] * p["smaj_cps"] > m // 512 + 1, p   # a short last slab
    monkeypatch.setenv("BSN_PLAN_CUS", "4")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gb = images(n, na16)
    rng = np.random.default_rng(wgx + S)
    ic = None if col0 == 0 else np.arange(col0, M)
    op = ba.ScaledOp(gb, None, ic, rng.uniform(0.1, 1.9, m), rng.uniform(0.3, 1.0, m), slices=S)
    X, Y = ba.DeviceArray.from_numpy(rng.normal(size=(m, 16))), ba.DeviceArray(n, 16)
    op.prod(X, Y)
    sync()
    got, ran = Y.to_numpy(), op.last_kernel()
    monkeypatch.setenv("BSN_NO_SMAJ", "1")
    op.prod(X, Y)
    sync()
    ref, ran_ref = Y.to_numpy(), op.last_kernel()
    op.close()
    assert template_args(ran) == want, ran
    assert "k_prod<" in ran_ref, ran_ref
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    np.testing.assert_array_equal(got, ref)


def test_whole_solve_is_bit_identical(ba, monkeypatch):
    """bed_randomSVD on the first shape, its product passes (warm start included) on the whole-round grid: d, u, v of the
    solve without the sample-major copy"""
    n, k = 4645, 10
    monkeypatch.setenv("BSN_PLAN_CUS", "4")
    gb = ba.bed.synthetic(n, M, seed=5)
    monkeypatch.setenv("BSN_NO_SMAJ", "1")
    ref = ba.bed_randomSVD(gb, k=k, block=16)
    assert ref["tiled"] == 0 and ref["converged"]
    monkeypatch.delenv("BSN_NO_SMAJ")
    assert gb.sample_major()
    res = ba.bed_randomSVD(gb, k=k, block=16)
    assert res["tiled"] == 2 and res["converged"]
    for f in ("d", "u", "v", "center", "scale"):
        np.testing.assert_array_equal(res[f], ref[f], err_msg=f)
    gb.close()
