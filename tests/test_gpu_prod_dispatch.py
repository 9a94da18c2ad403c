"""Which instance of the streaming kernels a product takes (bigsnpr_amd/csrc/prod_plan.hpp: plan_prod, choose_cprod,
choose_prod, choose_prodT, launched by matvec.hip) and that it computes the same bits as the product on the variant-major image
(BSN_NO_SMAJ=1), asserted with assert_array_equal as tests/test_gpu_smaj.py does.  The expected names are those the launch
ladders of matvec.hip reported for these calls before the choice was moved into prod_plan.hpp (tools/probe_prod_paths.py,
profiles/prod_dispatch_refactor.txt).  Shapes: 1 100 samples (two 1024-sample workgroups of k_prod, three 512-sample ones of
k_prodT, the last ragged) x 2 100 variants (a ragged last step and chunk, several slabs).
k_cprod<NB, NPLANE, KC, RAW0, STATS, CONTIG, TILES, WAVES, MINW, TAG, TILED, SGB, NASKIP>, k_prod<NB, CONTIG, RAWP, HASQ, TAG,
TILED>, k_prodT<NB, HASQ, TILES, WAVES, TAG, SGB, NASKIP, SPARSE>, k_prod8<NB, HASNA, CONTIG>."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M = 1100, 2100


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def make(ba, kind):
    """1 % missing values with the sample-major copy ("na"); the same with the streaming-layout copy instead ("tiled"); complete data"""
    g = ba.bed.synthetic(N, M, seed=42 if kind == "complete" else 41, na16=0 if kind == "complete" else 655)
    assert g.tile() if kind == "tiled" else g.sample_major()
    return g


@pytest.fixture(scope="module")
def images(ba):
    im = {kind: make(ba, kind) for kind in ("na", "tiled")}
    yield im
    for g in im.values():
        g.close()


def product(ba, monkeypatch, image, ic, nv, S, env=()):
    """(Y, kernel) of A~ X in the given environment, and Y under BSN_NO_SMAJ=1 as well"""
    rng = np.random.default_rng(nv * 100 + S)
    m = M if ic is None else ic.size
    X = ba.DeviceArray.from_numpy(rng.normal(size=(m, nv)))
    op = ba.ScaledOp(image, None, ic, rng.uniform(0.1, 1.9, m), rng.uniform(0.3, 1.0, m), slices=S)
    for k, v in env:
        monkeypatch.setenv(k, v)
    Y = op.prod(X)
    op.sync()
    got, kernel = Y.to_numpy(), op.last_kernel().replace("void bsn::", "")
    monkeypatch.setenv("BSN_NO_SMAJ", "1")
    Y = op.prod(X)
    op.sync()
    ref, ref_kernel = Y.to_numpy(), op.last_kernel()
    monkeypatch.delenv("BSN_NO_SMAJ")
    for k, _ in env:
        monkeypatch.delenv(k)
    op.close()
    assert "k_prodT" not in ref_kernel
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    np.testing.assert_array_equal(got, ref)
    return kernel


SCATTERED = np.sort(np.random.default_rng(5).permutation(M)[:1500])
NO_SKIP = (("BSN_NA_SKIP", "0"),)   # (the host rule may take the skipping kernels on an image this small: switched off where the name is pinned)
# image, ind_col, vectors, slices, environment -> the kernel of the product
PRODUCTS = [
    ("NB=1 contiguous", "na", None, 8, 2, NO_SKIP, "k_prod<1, true, true, true, 0, false>"),
    ("NB=1 gathered", "na", SCATTERED, 8, 2, NO_SKIP, "k_prod<1, false, true, true, 0, false>"),
    ("NB=1 tiled", "tiled", None, 8, 2, NO_SKIP, "k_prod<1, true, true, true, 0, true>"),
    ("NB=2 on k_prod", "na", SCATTERED, 16, 2, NO_SKIP, "k_prod<2, false, true, true, 0, false>"),
    ("k_prodT<2>", "na", None, 16, 2, NO_SKIP, "k_prodT<2, true, 2, 16, 0, 3, false, false>"),
    ("sparse k_prodT<3>", "na", None, 16, 3, NO_SKIP, "k_prodT<3, true, 2, 16, 0, 3, false, true>"),
    ("dense k_prodT<3>", "na", None, 16, 3, NO_SKIP + (("BSN_NO_SPARSE_PROD", "1"),), "k_prodT<3, true, 2, 16, 0, 3, false, false>"),
    ("56-bit panel", "na", None, 5, 7, NO_SKIP, "k_prodT<3, true, 2, 16, 0, 3, false, false>"),
    ("NASKIP k_prodT<2>", "na", None, 16, 2, (("BSN_NA_SKIP", "1"),), "k_prodT<2, true, 2, 16, 0, 0, true, false>"),
    ("NASKIP k_prodT<3>", "na", None, 16, 3, (("BSN_NA_SKIP", "1"),), "k_prodT<3, true, 2, 16, 0, 0, true, false>"),
    # col0 = 64 is no chunk boundary of the copy: 48 digit columns go as two launches of k_prod (10 + 6 vectors)
    ("col0=64, 48 columns", "na", np.arange(64, M), 16, 3, NO_SKIP, "k_prod<2, true, true, true, 0, false>"),
]


@pytest.mark.parametrize("name,image,ic,nv,S,env,want", PRODUCTS, ids=[p[0] for p in PRODUCTS])
def test_product_kernel(ba, monkeypatch, images, name, image, ic, nv, S, env, want):
    assert product(ba, monkeypatch, images[image], ic, nv, S, env) == want


def streaming_kernels(gb):
    from bigsnpr_amd import _lib
    buf = C.create_string_buffer(8192)
    _lib.check(_lib.load().bsn_bed_streaming_kernels(gb.handle, buf, 8192))
    return {k: v.replace("void bsn::", "") for k, v in (line.split("=", 1) for line in buf.value.decode().splitlines() if "=" in line)}


def solve_both_ways(ba, monkeypatch, gb, **kw):
    r = ba.bed_randomSVD(gb, k=3, **kw)
    names = streaming_kernels(gb)
    monkeypatch.setenv("BSN_NO_SMAJ", "1")
    ref = ba.bed_randomSVD(gb, k=3, **kw)
    monkeypatch.delenv("BSN_NO_SMAJ")
    for f in ("d", "u", "v"):
        np.testing.assert_array_equal(r[f], ref[f], err_msg=f)
    return names


def test_crossproduct_kernels_of_a_solve(ba, monkeypatch):
    """the crossproduct's instance is visible through a solve (bsn_bed_streaming_kernels); fresh handles: the first solve counts"""
    images = {kind: make(ba, kind) for kind in ("na", "tiled")}
    monkeypatch.setenv("BSN_NA_SKIP", "0")
    k = solve_both_ways(ba, monkeypatch, images["na"])
    assert k["cprod"] == "k_cprod<1, 2, 512, true, false, true, 2, 8, 1, 0, false, 0, false>"
    assert k["cprod_stats"] == "k_cprod<1, 2, 512, true, true, true, 2, 8, 1, 0, false, 0, false>"
    assert k["prod"] == "k_prod<1, true, true, true, 0, false>"
    k = solve_both_ways(ba, monkeypatch, images["tiled"])
    assert k["cprod"] == "k_cprod<1, 2, 512, true, false, true, 4, 8, 1, 0, true, 0, false>"   # 4 tiles per wave on the tiled copy
    assert k["cprod_stats"] == "k_cprod<1, 2, 512, true, true, true, 2, 8, 1, 0, true, 0, false>"   # the counting pass keeps 2
    assert k["prod"] == "k_prod<1, true, true, true, 0, true>"
    monkeypatch.setenv("BSN_NA_SKIP", "1")
    k = solve_both_ways(ba, monkeypatch, images["na"], block=16)
    assert k["cprod"] == "k_cprod<2, 2, 512, true, false, true, 2, 16, 1, 0, false, 0, true>"
    assert k["prod"] == "k_prodT<2, true, 2, 16, 0, 0, true, false>"
    assert k["cprod_wide"] == "k_cprod<3, 2, 512, true, false, true, 2, 16, 1, 0, false, 0, true>"
    assert k["prod_wide"] == "k_prodT<3, true, 2, 16, 0, 0, true, false>"


def test_complete_data_drops_the_missing_value_plane(ba, monkeypatch):
    """once the counting pass has found no missing value: NPLANE = 1, HASQ = false"""
    images = {"complete": make(ba, "complete")}
    k = solve_both_ways(ba, monkeypatch, images["complete"])
    assert k["cprod"] == "k_cprod<1, 1, 512, true, false, true, 2, 8, 1, 0, false, 0, false>"
    assert k["prod"] == "k_prod<1, true, true, false, 0, false>"
    k = solve_both_ways(ba, monkeypatch, images["complete"], block=16)
    assert k["cprod"] == "k_cprod<2, 1, 512, true, false, true, 2, 16, 1, 0, false, 3, false>"
    assert k["prod"] == "k_prodT<2, false, 2, 16, 0, 3, false, false>"
    assert k["cprod_wide"] == "k_cprod<3, 1, 512, true, false, true, 2, 16, 1, 0, false, 3, false>"
    assert k["prod_wide"] == "k_prodT<3, false, 2, 16, 0, 3, false, false>"


def test_byte_image(ba, monkeypatch):
    """k_prod8 by name; k_cprod8 has no name to report, its crossproduct is checked against fp64"""
    rng = np.random.default_rng(3)
    n, m = 300, 700
    dos = rng.integers(7, 208, size=(n, m)).astype(np.uint8)
    dos_na = dos.copy()
    dos_na[rng.random(dos.shape) < 0.03] = 3
    for d, has_na in ((dos, "false"), (dos_na, "true")):
        G = ba.FBM_code256(d, ba.CODE_DOSAGE)
        for ic, contig in ((None, "true"), (np.sort(rng.permutation(m)[:500]), "false")):
            for nv, nb in ((8, 1), (16, 2)):
                assert product_m(ba, monkeypatch, G._bed, m, ic, nv) == "k_prod8<%d, %s, %s>" % (nb, has_na, contig)
    G = ba.FBM_code256(dos, ba.CODE_DOSAGE)
    y = rng.normal(size=n)
    vals = ba.CODE_DOSAGE[dos.astype(np.int64)]
    z = ba.big_cprodVec(G, y)
    ref = vals.T @ y
    assert np.abs(z - ref).max() <= 1e-9 * np.abs(ref).max()


def product_m(ba, monkeypatch, image, m_all, ic, nv):
    rng = np.random.default_rng(nv)
    m = m_all if ic is None else ic.size
    X = ba.DeviceArray.from_numpy(rng.normal(size=(m, nv)))
    op = ba.ScaledOp(image, None, ic, rng.uniform(0.1, 1.9, m), rng.uniform(0.3, 1.0, m), slices=2)
    Y = op.prod(X)
    op.sync()
    got, kernel = Y.to_numpy(), op.last_kernel().replace("void bsn::", "")
    monkeypatch.setenv("BSN_NO_SMAJ", "1")
    Y = op.prod(X)
    op.sync()
    monkeypatch.delenv("BSN_NO_SMAJ")
    np.testing.assert_array_equal(got, Y.to_numpy())
    op.close()
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    return kernel
