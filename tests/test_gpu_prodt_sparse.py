"""k_prodT's sparse form (bigsnpr_amd/csrc/prodt_sparse.hpp: the code plane and the missing-value plane in ONE
v_smfmac_i32_16x16x128_i8) against the dense two-plane kernels (BSN_NO_SPARSE_PROD=1) and against k_prod on the
variant-major image (BSN_NO_SMAJ=1): the same integers per sample, so every product and a whole solve are compared
with assert_array_equal.  Only 16 vectors x 3 slices (three column blocks of 24-bit panels) take the sparse form, and
every product checks by the launched kernel's name that it did; the two-block cases (16 and 11 vectors x 2 slices) and
5 vectors x 7 slices compare the dense kernel with itself and with k_prod — they pin the dispatch, not the sparse form.  The images come from bed.from_payload, so the missing pattern is the test's:
  - the four combinations (present / missing x present / missing) in every pair position of a dword of the copy
    (16 consecutive variants of one sample), each in its own dword of rows 0 .. 7;
  - a dword with all 16 missing (row 8), a whole sample row missing (row 9), whole variants missing (7 and m - 1);
  - 2 % scattered missing values everywhere else; and an image without any that still takes the missing-value plane.
Panels: integers that make the quantiser's scale exactly 1 and put the digits at the ends of int8 — the digits of B at
-127 / 127 in the top slice (the 0.99 headroom of the scale excludes -128 there) and -128 / 127 in the lower ones, those
of A at -128 / 127 in the lower slices and as high in the top slice as max(|b|, |b - 3 a|) <= scale admits (|a| <= 2/3
of it, at centre 1.5) —, a centre of 2.0 throughout (B = 2 A, the largest B the scale admits), and random ones.
Shapes: samples short of a tile (17) and of a workgroup (513, 1000); variants: a ragged last chunk, one slab and several
(513, 1537, 20000); a chunk-aligned sub-range of the variants."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLINK = np.array([3, 2, 0, 1], dtype=np.uint8)   # genotype 0 / 1 / 2 / missing -> the .bed code


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def payload_of(G):
    """G [n x m] in {0, 1, 2, 3 = missing} -> the .bed payload (variant-major, four samples per byte)"""
    n, m = G.shape
    nb = (n + 3) // 4
    c = np.zeros((4 * nb, m), dtype=np.uint8)
    c[:n] = PLINK[G]
    c = c.reshape(nb, 4, m)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).T.copy().ravel()


def crafted(n, m, seed):
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 3, (n, m)).astype(np.uint8)
    G[rng.random((n, m)) < 0.02] = 3
    for p in range(8):                      # pair position p of dword 1 + c, sample row p: combination c
        for c in range(4):
            j = 16 * (1 + c)
            G[p, j:j + 16] = rng.integers(0, 3, 16)
            G[p, j + 2 * p] = 3 if c & 1 else rng.integers(0, 3)
            G[p, j + 2 * p + 1] = 3 if c & 2 else rng.integers(0, 3)
    G[8, 320:336] = 3                       # a dword with all 16 missing
    G[9, :] = 3                             # a sample without a genotype
    G[:, 7] = 3                             # variants without a genotype: inside a dword, and the last one
    G[:, m - 1] = 3
    return G


def extreme_panel(m, nv, S, rng):
    """X [m x nv] of integers, centre [m]: with scale 1 the quantiser's scale is exactly 1 (max(|b|) = the largest
    integer M with M <= 0.99 * 2^(8 S - 1), M even), so A = a and B = c a are these integers"""
    M = int(0.99 * 2.0 ** (8 * S - 1)) & ~1
    top = 256 ** (S - 1)
    hi, lo = sum(127 * 256 ** s for s in range(S - 1)), sum(-128 * 256 ** s for s in range(S - 1))
    ce = rng.uniform(0.2, 1.9, m)
    a = rng.integers(-M // 3, M // 3, m).astype(np.float64)
    rows = [(2.0, M // 2), (2.0, -(M // 2)),                         # B = +-M: top digit +-127
            (2.0, (127 * top + lo) // 2),                            # B: top digit 127, lower digits -128
            (1.5, -((127 * top - hi) // 3) * 2),                     # B = -(127 top - hi) or next to it: top -127, lower 127
            (1.0, hi + 60 * top), (1.0, lo - 60 * top), (1.0, lo + 60 * top), (1.0, hi - 60 * top),   # A = B: lower digits at both ends
            (1.5, int(M / 1.5)), (1.5, -int(M / 1.5))]               # the largest |A| the scale admits
    for k, (c, v) in enumerate(rows):
        for j in (16 + 2 * k, 335 - k, m - 1 - k):                   # in the crafted dwords, the all-missing dword, the ragged tail
            ce[j], a[j] = c, v
    X = a[:, None] * np.where(np.arange(nv) % 2 == 0, 1.0, -1.0)[None, :]
    X[:, nv - 1] = np.roll(a, 3)                                     # (one vector with other neighbours, and whatever scale that gives)
    return X, ce


def three_ways(ba, monkeypatch, op, X, n):
    from bigsnpr_amd import _lib
    sync = _lib.load().bsn_device_sync
    Xd, Y = ba.DeviceArray.from_numpy(X), ba.DeviceArray(n, X.shape[1])
    out = {}
    for tag, env in (("sparse", None), ("dense", "BSN_NO_SPARSE_PROD"), ("k_prod", "BSN_NO_SMAJ")):
        if env:
            monkeypatch.setenv(env, "1")
        op.prod(Xd, Y)
        sync()
        out[tag] = Y.to_numpy()
        out[tag + " kernel"] = op.last_kernel()
        if env:
            monkeypatch.delenv(env)
    return out


def compare(ba, monkeypatch, gb, n, m, seed, complete=False):
    rng = np.random.default_rng(seed)
    assert gb.sample_major()
    # The kernels that skip the plane of K-steps without a missing code keep their precedence over the sparse form, and
    # the host rule takes them on images as small as these (the padding rows of a 17-sample image are free steps): this
    # file is about the sparse form, so the rule is switched off here.  tests/test_gpu_na_skip.py has the other side.
    monkeypatch.setenv("BSN_NA_SKIP", "0")
    subs = [None] + ([np.arange(512, m - 7)] if m - 7 > 512 + 400 else [])
    # (5 x 7 slices: three column blocks of 56-bit panels, whose slice sums pass 2^53 — the dispatch keeps them dense)
    for nv, S in ((16, 2), (11, 2), (16, 3), (5, 7)):
        Xe, ce_e = extreme_panel(m, nv, min(S, 3), rng)
        panels = ([("extreme digits", Xe, ce_e, np.ones(m))] if S <= 3 else []) + [
                  ("centre 2", rng.normal(size=(m, nv)), np.full(m, 2.0), rng.uniform(0.3, 1.0, m)),
                  ("random", rng.normal(size=(m, nv)), rng.uniform(0.1, 1.9, m), rng.uniform(0.3, 1.0, m))]
        for ic in subs:
            for what, X, ce, sa in panels:
                if ic is not None and what == "extreme digits":
                    continue                                          # (its scale is built on the whole range)
                cc, ss, XX = (ce, sa, X) if ic is None else (ce[ic], sa[ic], X[ic])
                op = ba.ScaledOp(gb, None, ic, cc, ss, slices=S)
                r = three_ways(ba, monkeypatch, op, XX, n)
                msg = "n=%d m=%d nv=%d slices=%d %s%s" % (n, m, nv, S, what, "" if ic is None else " sub-range")
                assert np.isfinite(r["sparse"]).all() and np.abs(r["sparse"]).max() > 0, msg
                # what ran: the sparse k_prodT<3> for 24-bit panels in the default environment, dense kernels otherwise
                assert "k_prodT<%d," % (2 if nv * S <= 32 else 3) in r["sparse kernel"], (msg, r["sparse kernel"])
                assert sparse_arg(r["sparse kernel"]) == ((nv, S) == (16, 3)), (msg, r["sparse kernel"])
                assert "k_prodT<" in r["dense kernel"] and not sparse_arg(r["dense kernel"]), (msg, r["dense kernel"])
                assert "k_prod<" in r["k_prod kernel"], (msg, r["k_prod kernel"])
                np.testing.assert_array_equal(r["sparse"], r["dense"], err_msg=msg + ": sparse against dense k_prodT")
                np.testing.assert_array_equal(r["sparse"], r["k_prod"], err_msg=msg + ": sparse against k_prod")
                if what == "extreme digits" and not complete:
                    # the scale is 1: row 9 (every genotype missing) is sum_j B_j - sum_j B_j = 0, exactly
                    assert np.all(r["sparse"][9] == 0.0), msg
                op.close()


@pytest.mark.parametrize("n", [17, 513, 1000])
@pytest.mark.parametrize("m", [513, 1537, 20000])
def test_sparse_product_is_bit_identical(ba, monkeypatch, n, m):
    G = crafted(n, m, seed=n + m)
    gb = ba.bed.from_payload(payload_of(G), n, m)
    got = gb[:, :64]                                      # (the pattern is the one asked for: NA reads back as -1)
    np.testing.assert_array_equal(got == -1, G[:, :64] == 3)
    compare(ba, monkeypatch, gb, n, m, seed=3 * n + m)
    gb.close()


def test_image_without_missing_values_on_the_missing_value_plane(ba, monkeypatch):
    n, m = 513, 1537
    G = np.random.default_rng(1).integers(0, 3, (n, m)).astype(np.uint8)
    gb = ba.bed.from_payload(payload_of(G), n, m)
    monkeypatch.setenv("BSN_FORCE_NA_PLANE", "1")         # (no count has run on this handle; the switch makes it certain)
    compare(ba, monkeypatch, gb, n, m, seed=8, complete=True)
    gb.close()


def kernels(gb):
    import ctypes as C
    from bigsnpr_amd import _lib
    buf = C.create_string_buffer(8192)
    _lib.check(_lib.load().bsn_bed_streaming_kernels(gb.handle, buf, 8192))
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines() if "=" in line)


def sparse_arg(name):
    """k_prodT<NB, HASQ, TILES, WAVES, TAG, SGB, NASKIP, SPARSE>: the last argument"""
    assert "k_prodT<" in name, name
    return name.split("<", 1)[1].rstrip("> ").split(",")[7].strip() == "true"


def test_whole_solve_with_the_switch_on_and_off(ba, monkeypatch):
    n, m, k = 2500, 300000, 20
    gb = ba.bed.synthetic(n, m, seed=5, na16=655)
    assert gb.sample_major()
    res = ba.bed_randomSVD(gb, k=k, block=16)
    names = kernels(gb)
    assert res["tiled"] == 2 and res["converged"]
    ran = [v for v in names.values() if "k_prodT<" in v]
    nb = lambda v: int(v.split("<", 1)[1].split(",")[0])                    # noqa: E731
    # (the three-block launches take the sparse form; with two blocks it measured slower and the dense kernel stays)
    assert {nb(v) for v in ran} == {2, 3} and all(sparse_arg(v) == (nb(v) == 3) for v in ran), names
    monkeypatch.setenv("BSN_NO_SPARSE_PROD", "1")
    ref = ba.bed_randomSVD(gb, k=k, block=16)
    names = kernels(gb)
    monkeypatch.delenv("BSN_NO_SPARSE_PROD")
    ran = [v for v in names.values() if "k_prodT<" in v]
    assert len(ran) >= 2 and not any(sparse_arg(v) for v in ran), names
    for f in ("d", "u", "v", "center", "scale"):
        np.testing.assert_array_equal(res[f], ref[f], err_msg=f)
    assert (res["niter"], res["nops"]) == (ref["niter"], ref["nops"])
    gb.close()
