"""snp_fastImpute on the device (bsn_fast_impute, bigsnpr_amd/csrc/fastimpute.hip) against the CPU statement
(tests/native/fastimpute_ref.cpp, compiled from the same fastimpute_step.hpp).  Bytes, image and infos are compared
exactly: on the masked example.bed case of the reference's own test through the host mirror, and through the entry
point with hand-made predictor lists on sample counts around the constants of the kernel (read from its source),
predictor counts around a feature turn, more targets than the grid, and the variants that are no target."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import fastimpute_inputs as fi  # noqa: E402
import fastimpute_ref as ref  # noqa: E402
from impute_inputs import same_image  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = fi.SEED
K = fi.kernel_constants()


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def raw_call(ba, handle, n, m, off, idx, p_train, seed):
    """bsn_fast_impute itself: (status, result handle, bytes, infos, n_all_missing)"""
    from bigsnpr_amd import _lib
    off, idx = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(idx, dtype=np.int32)
    out = np.empty((n, m), dtype=np.uint8, order="F")
    infos = np.empty((2, m), dtype=np.float64)
    h, n_all = C.c_void_p(), C.c_int64(-1)
    st = _lib.load().bsn_fast_impute(handle, off.ctypes.data_as(_lib.i64p), idx.ctypes.data_as(_lib.i32p), float(p_train),
                                     int(seed), C.byref(h), out.ctypes.data_as(_lib.u8p), infos.ctypes.data_as(_lib.f64p),
                                     C.byref(n_all))
    return st, h, out, infos, int(n_all.value)


def device(ba, g, preds, p_train=0.8, seed=SEED):
    """the entry point on FBM bytes g with the predictor lists preds: an FBM_code256 with .bytes, .infos, .n_all_missing"""
    n, m = g.shape
    src = ba.FBM_code256(g)
    before = src._bed.download()
    off, idx = ref.lists(preds)
    st, h, out, infos, n_all = raw_call(ba, src.handle, n, m, off, idx, p_train, seed)
    assert st == 0, ba.load().bsn_last_error().decode()
    res = ba.FBM_code256._from_handle(h, n, m, ba.CODE_IMPUTE_PRED)
    res.bytes, res.infos, res.n_all_missing = out, infos, n_all
    np.testing.assert_array_equal(src._bed.download(), before)   # the source is untouched
    return res


def against_the_statement(ba, g, preds, p_train=0.8, seed=SEED):
    want, want_infos, want_all = ref.fast_impute(g, *ref.lists(preds), p_train, seed, nthreads=8)
    res = device(ba, g, preds, p_train, seed)
    np.testing.assert_array_equal(res.bytes, want)
    np.testing.assert_array_equal(res.infos, want_infos)          # NaN in the same places, equal elsewhere
    assert res.n_all_missing == want_all == int((g == 3).all(0).sum())
    assert res._has_na == (want_all > 0)
    same_image(ba, res)                                           # the image is what bsn_fbm_open makes of these bytes
    return res


def nearest(m, count):
    """for each variant the `count` nearest other variants, ascending"""
    out = []
    for j in range(m):
        others = sorted((k for k in range(m) if k != j), key=lambda k: (abs(k - j), k))[:count]
        out.append(np.array(sorted(others), dtype=np.int32))
    return out


def edge_image(n, m, seed):
    """about 10 % missing; variants 0 and m - 1 are targets where n allows, 2 has no observed call, 3 a single one, 5 has
    no missing call and lies between the targets 4 and 6"""
    g = fi.random_image(n, m, seed, missing=0.1)
    rng = np.random.default_rng(seed + 1)
    if n >= 2:
        for j in (0, 4, 6, m - 1):
            g[:, j] = np.where(g[:, j] == 3, rng.integers(0, 3, n), g[:, j])
            g[rng.integers(0, n), j] = 3
    g[:, 2] = 3
    g[:, 3] = 3
    g[n // 2, 3] = 1
    g[:, 5] = rng.integers(0, 3, n)
    return np.asfortranarray(g)


# ---- 1. example data through the host mirror ----------------------------------------------------------------------------------
def test_example_data(ba):
    """test-3-fastImpute.R:21-64: the device's bytes, image and infos equal the CPU statement's, given the predictor lists
    the mirror built from snp_cor on the device; the reference's F test and the comparison with `mode` hold on them"""
    ex = fi.example_case()
    G, G0, ind = ex["G"], ex["G0"], ex["ind"]
    src = ba.FBM_code256(G)
    before = src._bed.download()
    res = ba.snp_fastImpute(src, ex["chr"], p_train=0.6, seed=SEED, return_bytes=True)
    np.testing.assert_array_equal(src._bed.download(), before)
    lens = np.diff(res.pred_off)
    assert (lens[ind] >= 5).all() and res.pred_idx.size == res.pred_off[-1]
    want, want_infos, want_all = ref.fast_impute(G, res.pred_off, res.pred_idx, 0.6, SEED, nthreads=8)
    np.testing.assert_array_equal(res.bytes, want)
    np.testing.assert_array_equal(res.infos, want_infos)
    assert res.n_all_missing == want_all == 0 and res.seed == SEED and not res._has_na
    same_image(ba, res)                                           # .bytes are the image's bytes
    # the reference's expectations on the device's result
    mask = G[:, ind] == 3
    nb_err = ((res.bytes[:, ind] - 4 != G0[:, ind]) & mask).sum(0)
    F, p, slope = fi.f_test_through_origin(nb_err, res.infos[0, ind] * res.infos[1, ind] * ex["n"])
    print("F", F, "p", p, "slope", slope, "errors", nb_err.sum() / mask.sum())
    assert p < 2e-16
    # the consumers of complete data run on the result
    counts = ba.bed_counts(res._bed)
    assert (counts[3] == 0).all() and np.array_equal(counts[:3, ind].sum(0), np.full(ind.size, ex["n"]))
    x = np.random.default_rng(1).integers(-3, 4, ex["m"]).astype(np.float64)
    assert np.isfinite(ba.bed_prodVec(res._bed, x)).all()
    again = ba.snp_fastImputeSimple(res._bed, "mode")
    np.testing.assert_array_equal(again._bed.download(), res._bed.download())   # nothing is left to impute
    # a bed is accepted as well
    from_bed = ba.snp_fastImpute(ba.bed(os.path.join(fi.GOLDEN, "example-missing.bed")), np.ones(500), seed=SEED, size=20)
    assert from_bed.infos.shape == (2, 500) and (ba.bed_counts(from_bed._bed)[3] == 0).all()


# ---- 2. edge shapes through the entry point -----------------------------------------------------------------------------------
SHAPES = [(1, 0), (15, 1), (16, 4), (17, 5), (63, K["kFeatTurn"] + 1), (65, 400),
          (K["kTurnSamples"] + 1, 5), (2 * K["kTurnSamples"] + 1, K["kFeatTurn"] + 1),
          (K["kLdsSamples"], 4), (K["kLdsSamples"] + 1, K["kFeatTurn"] + 1)]


@pytest.mark.parametrize("n,npred", SHAPES)
def test_edge_shapes(ba, n, npred):
    """sample counts around a dword, a wave, one and two workgroup turns and the switch from LDS to global scratch;
    predictor counts 0, 1, 4, 5, one more than a feature turn, and 2 x size of the default"""
    m = max(12, npred + 3)
    g = edge_image(n, m, 7 * n + npred)
    res = against_the_statement(ba, g, nearest(m, npred))
    if n >= 17:
        assert (res.bytes[:, 2] == 3).all() and np.isnan(res.infos[1, [2, 5]]).all() and res.infos[0, 2] == 1 and res.infos[0, 5] == 0
        assert (res.bytes[:, 3] >= 4).sum() == n - 1 and np.isnan(res.infos[1, 3])   # its one call trains, drawn or not
        assert 0 < res.infos[0, 0] < 1 and 0 < res.infos[0, m - 1] < 1


def test_more_targets_than_the_grid(ba):
    """a workgroup takes a second target, with other roles, another margin and another list"""
    m = K["kGridTargets"] + 70
    g = fi.random_image(19, m, 5, missing=0.15)
    res = against_the_statement(ba, g, fi.window_lists(m, 2))
    assert ((g == 3).any(0) & ~(g == 3).all(0)).sum() > K["kGridTargets"]
    assert res.bytes.shape == (19, m)


def test_p_train_one_and_nobody_training(ba):
    """p_train = 1: nobody validates; p_train tiny: nobody draws a training role, every observed sample trains"""
    g = edge_image(70, 12, 3)
    for p_train in (1.0, 1e-12):
        res = against_the_statement(ba, g, nearest(12, 5), p_train=p_train)
        assert np.isnan(res.infos[1]).all()


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------
def test_determinism(ba):
    m = 40
    g = fi.random_image(300, m, 12, missing=0.1)
    preds = nearest(m, 9)
    a, b = device(ba, g, preds), device(ba, g, preds)
    np.testing.assert_array_equal(a.bytes, b.bytes)
    np.testing.assert_array_equal(a.infos, b.infos)
    np.testing.assert_array_equal(a._bed.download(), b._bed.download())
    other = [p if j == 7 else p[:2] for j, p in enumerate(preds)]   # every list but one target's changes
    c = device(ba, g, other)
    np.testing.assert_array_equal(c.bytes[:, 7], a.bytes[:, 7])
    assert c.infos[1, 7] == a.infos[1, 7] and not np.array_equal(c.bytes, a.bytes)
    d = device(ba, g, preds, seed=SEED + 1)
    assert not np.array_equal(d.bytes, a.bytes)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ba, golden_dir, monkeypatch):
    L = ba.load()
    g = fi.random_image(50, 6, 2)
    n, m = g.shape
    G = ba.FBM_code256(g)
    off, idx = ref.lists(nearest(m, 2))

    def refused(handle, off, idx, p_train=0.8, n=n, m=m):
        st, h, *_ = raw_call(ba, handle, n, m, off, idx, p_train, SEED)
        assert st != 0 and not h.value
        return L.bsn_last_error().decode()

    D = ba.FBM_code256(np.where(g < 3, g + 4, 3).astype(np.uint8), ba.CODE_DOSAGE)
    assert D.bits == 8
    msg = refused(D.handle, off, idx)
    assert "2-bit genotype image" in msg and "snp_fastImpute" in msg
    for p_train in (0.0, -0.1, 1.5, float("nan")):
        assert "'p_train' must lie in (0, 1]" in refused(G.handle, off, idx, p_train)
    own = idx.copy()
    own[off[3]] = 3
    assert "variant 3 is named as its own predictor" in refused(G.handle, off, own)
    for bad in (-1, m):
        outside = idx.copy()
        outside[off[2] + 1] = bad
        assert "lies outside [0, %d)" % m in refused(G.handle, off, outside)
    # an out-of-core source
    path = os.path.join(golden_dir, "example-missing.bed")
    res = ba.bed(path)
    pitch = (res.nrow + 3) // 4 + 255 & ~255
    monkeypatch.setenv("BSN_IMAGE_BUDGET", str(130 * pitch))
    ooc = ba.bed(path)
    monkeypatch.delenv("BSN_IMAGE_BUDGET")
    assert ooc.streamed
    msg = refused(ooc.handle, *ref.lists(fi.window_lists(500, 2)), n=200, m=500)
    assert "snp_fastImpute needs the genotype image resident" in msg
    # the mirror's own
    with pytest.raises(ValueError, match="CODE_012"):
        ba.snp_fastImpute(D, np.ones(m))
    with pytest.raises(ValueError, match="Incompatibility between dimensions."):
        ba.snp_fastImpute(G, np.ones(m + 1))
    # and the call still works afterwards
    against_the_statement(ba, g, nearest(m, 2))
