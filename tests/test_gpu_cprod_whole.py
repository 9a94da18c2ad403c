"""k_cprod's one-dimensional grid (bigsnpr_amd/csrc/prod_plan.hpp: plan_cprod, cprod_slab): the blocks of variants that fill
whole rounds of the CUs run as one workgroup over all samples, the blocks beyond the last whole round are cut along the samples
into slabs, and k_cprod_final adds the slabs' partial sums.  A few thousand variants never fill a round of the device's CUs, so
every case runs with BSN_PLAN_CUS=4; how many workgroups of an instance a CU holds is the runtime's answer, so the variant
counts are made from what bsn_op_cprod_grid reports (whole rounds of 4 x resident workgroups).  At 2 000 - 5 000 samples a
slab's partial sums cost more than the rule lets the fill gain for most shapes, so beside the rule's own count
(BSN_CPROD_SLABS unset) every case runs with counts of the caller that make the slab shapes the kernel can go wrong at.  The
geometry of every run is asserted — against the planner on the CPU (tests/native/cprod_grid_ref.cpp) — before the GPU runs
it, and Z is compared bit for bit with the same call under BSN_CPROD_ONE_SPLIT=1 (one workgroup per block, the sums as they
always were)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

CUS = 4
# samples -> chunks of 512; slab counts asked for -> (slabs, chunks per slab) they must give
#   4645: 10 chunks, the last ragged (37 samples).  4 -> 4 x 3: an odd number of chunks, slabs from chunks 0, 3, 6, 9 (even and
#         odd), a short last slab of ONE chunk;  10 -> 10 x 1: every slab one chunk;  3 -> 3 x 4: a short last slab of two
#   2049: 6 chunks (a row is padded to 1 024 samples), the fifth of 1 sample, the sixth all padding.  2 -> 2 x 3: three chunks,
#         then three from an odd chunk;  6 -> 6 x 1;  4 -> 3 x 2
SLABS = {4645: {4: (4, 3), 10: (10, 1), 3: (3, 4)}, 2049: {2: (2, 3), 6: (6, 1), 4: (3, 2)}}
# name -> samples, first variant, blocks of variants as (whole rounds, blocks beyond them, variants the last block lacks)
SHAPES = {
    "two rounds and two blocks": (4645, 0, (2, 2, 37)),
    "two rounds": (4645, 0, (2, 0, 0)),                      # no remainder: the grid as it was
    "less than a round": (2049, 0, (0, 3, 11)),              # the warm-start geometry: every block a remainder block
    "from variant 512": (4645, 512, (1, 1, 250)),
}
# name -> slices (16 vectors: column blocks), environment, missing genotypes per 65 536, planes
PANELS = {
    "16 x 8 bits": (1, {"BSN_NA_SKIP": "0"}, 655, 2),
    "16 x 16 bits": (2, {"BSN_NA_SKIP": "0"}, 655, 2),
    "16 x 24 bits": (3, {"BSN_NA_SKIP": "0"}, 655, 2),
    "complete data": (3, {}, 0, 1),
    "skipping kernels 16 bits": (2, {"BSN_NA_SKIP": "1"}, 655, 2),
    "skipping kernels 24 bits": (3, {"BSN_NA_SKIP": "1"}, 655, 2),
}
M_MAX = 512 + (2 * CUS * 4 + 2) * 512   # variants of an image: two rounds of 4 CUs x up to 4 resident workgroups, two blocks, col0


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def cprod_grid(ba):
    from bigsnpr_amd import _lib
    fn = _lib.load().bsn_op_cprod_grid
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    names = ("blocks", "blocks_whole", "slabs", "cps", "nchunks", "m_rem", "per_wg", "ncu", "resident")

    def grid(op, nvec):
        out = np.zeros(9, dtype=np.int64)
        _lib.check(fn(op._h, nvec, out.ctypes.data_as(C.c_void_p)))
        return dict(zip(names, (int(v) for v in out)))
    return grid


@pytest.fixture(scope="module")
def images(ba):
    """one image per (samples, missing rate), with its code counts (an operator learns from them that the data is complete)"""
    made = {}

    def get(n, na16):
        if (n, na16) not in made:
            gb = ba.bed.synthetic(n, M_MAX, seed=n + na16, na16=na16)
            ba.bed_counts(gb)
            made[(n, na16)] = gb
        return made[(n, na16)]
    yield get
    for gb in made.values():
        gb.close()


def make_op(ba, gb, col0, m, S, seed):
    rng = np.random.default_rng(seed)
    return ba.ScaledOp(gb, None, np.arange(col0, col0 + m), rng.uniform(0.1, 1.9, m), rng.uniform(0.3, 1.0, m), slices=S)


@pytest.mark.parametrize("panel", list(PANELS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_crossproduct_is_bit_identical_to_one_split(ba, images, cprod_grid, monkeypatch, shape, panel):
    import cprod_grid_ref as cg
    from bigsnpr_amd import _lib
    sync = _lib.load().bsn_device_sync
    n, col0, (rounds, beyond, lacks) = SHAPES[shape]
    S, env, na16, nplane = PANELS[panel]
    NB = S
    monkeypatch.setenv("BSN_PLAN_CUS", str(CUS))
    monkeypatch.setenv("BSN_NO_TILED", "1")      # (the tiled copy has its own kernels, which keep one workgroup per block)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gb = images(n, na16)
    # what a CU holds of this launch's instance: asked on any operator of the panel's shape
    probe = make_op(ba, gb, col0, 1024, S, 1)
    g0 = cprod_grid(probe, 16)
    probe.close()
    per_wg, resident = g0["per_wg"], g0["resident"]
    assert g0["ncu"] == CUS and per_wg == (256 if NB == 1 else 512) and 1 <= resident <= 4, g0
    slots = CUS * resident
    m = (rounds * slots + beyond) * per_wg - lacks
    assert col0 + m <= M_MAX
    op = make_op(ba, gb, col0, m, S, 7)
    rng = np.random.default_rng(rounds + beyond + S)
    X, Z = ba.DeviceArray.from_numpy(rng.normal(size=(n, 16))), ba.DeviceArray(m, 16)
    monkeypatch.setenv("BSN_CPROD_ONE_SPLIT", "1")
    g = cprod_grid(op, 16)
    assert (g["blocks"], g["blocks_whole"], g["slabs"], g["resident"]) == (rounds * slots + beyond,) * 2 + (0, 0), g
    op.cprod(X, Z)
    sync()
    ref = Z.to_numpy().copy()
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0 and (np.abs(ref).max(axis=1) > 0).mean() > 0.99
    monkeypatch.delenv("BSN_CPROD_ONE_SPLIT")
    split_runs = 0
    for want in [None] + list(SLABS[n]):
        if want is None:
            monkeypatch.delenv("BSN_CPROD_SLABS", raising=False)
        else:
            monkeypatch.setenv("BSN_CPROD_SLABS", str(want))
        # the geometry this run takes: the library's answer is the CPU planner's on the same facts, and the case's own
        f = cg.facts(n, m, NB, nplane=nplane, ncu=CUS, resident=resident, slabs=want or 0)
        p, g = cg.plan(**f), cprod_grid(op, 16)
        assert cg.check(**f) == 0
        assert {k: g[k] for k in ("blocks", "blocks_whole", "slabs", "cps", "nchunks", "m_rem")} == {
            k: p[k] for k in ("blocks", "blocks_whole", "slabs", "cps", "nchunks", "m_rem")}, (g, p)
        assert g["blocks"] == rounds * slots + beyond and g["nchunks"] == (n + 1023) // 1024 * 2
        if beyond == 0:
            assert (g["blocks_whole"], g["slabs"]) == (g["blocks"], 0), g          # whole rounds: nothing to cut
        elif want is not None:
            assert (g["blocks_whole"], g["slabs"], g["cps"]) == (rounds * slots,) + SLABS[n][want], g
            assert g["m_rem"] == beyond * per_wg - lacks
        split_runs += g["slabs"] > 0
        Z2 = ba.DeviceArray(m, 16)
        op.cprod(X, Z2)
        sync()
        np.testing.assert_array_equal(Z2.to_numpy(), ref, err_msg="BSN_CPROD_SLABS=%s %s" % (want, g))
    assert split_runs >= (len(SLABS[n]) if beyond else 0)
    op.close()


def test_the_rule_splits_a_lone_block(ba, images, cprod_grid, monkeypatch):
    """one block beyond two rounds of 16-bit panels: a quarter (or less) of the places taken, so the rule itself cuts it — into as
    many slabs as there are places, by the planner — and the sums are those of one workgroup per block"""
    import cprod_grid_ref as cg
    from bigsnpr_amd import _lib
    sync = _lib.load().bsn_device_sync
    n, S = 20000, 2                                  # (40 chunks: long enough for the rule to find that slabs pay)
    monkeypatch.setenv("BSN_PLAN_CUS", str(CUS))
    monkeypatch.setenv("BSN_NO_TILED", "1")
    monkeypatch.setenv("BSN_NA_SKIP", "0")
    gb = images(n, 655)
    probe = make_op(ba, gb, 0, 1024, S, 1)
    resident = cprod_grid(probe, 16)["resident"]
    probe.close()
    m = (2 * CUS * resident + 1) * 512 - 100
    op = make_op(ba, gb, 0, m, S, 3)
    g, p = cprod_grid(op, 16), cg.plan(**cg.facts(n, m, 2, ncu=CUS, resident=resident))
    assert g["slabs"] >= 2 and (g["blocks_whole"], g["slabs"], g["cps"], g["m_rem"]) == (
        2 * CUS * resident, p["slabs"], p["cps"], 412), (g, p)
    X = ba.DeviceArray.from_numpy(np.random.default_rng(11).normal(size=(n, 16)))
    got = op.cprod(X)
    sync()
    got = got.to_numpy().copy()
    monkeypatch.setenv("BSN_CPROD_ONE_SPLIT", "1")
    ref = op.cprod(X)
    sync()
    ref = ref.to_numpy()
    op.close()
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    np.testing.assert_array_equal(got, ref)


def test_whole_solve_is_bit_identical(ba, monkeypatch):
    """bed_randomSVD on the first shape (4 645 samples, two rounds of variants and two blocks at two and three column blocks if
    a CU holds one workgroup), its crossproduct passes — warm start included — on the new grid with four slabs for the
    remainder: d, u, v, center, scale of the solve with one workgroup per block"""
    n, k = 4645, 10
    m = (2 * CUS + 2) * 512 - 37
    monkeypatch.setenv("BSN_PLAN_CUS", str(CUS))
    monkeypatch.setenv("BSN_NO_TILED", "1")
    gb = ba.bed.synthetic(n, m, seed=5)
    monkeypatch.setenv("BSN_CPROD_ONE_SPLIT", "1")
    ref = ba.bed_randomSVD(gb, k=k, block=16)
    assert ref["converged"]
    monkeypatch.delenv("BSN_CPROD_ONE_SPLIT")
    monkeypatch.setenv("BSN_CPROD_SLABS", "4")
    res = ba.bed_randomSVD(gb, k=k, block=16)
    assert res["converged"]
    for f in ("d", "u", "v", "center", "scale"):
        np.testing.assert_array_equal(res[f], ref[f], err_msg=f)
    gb.close()
