"""The code counts of a handle over all samples stay on the device between calls (bsn_bed::stats_cache): the first solve
with bed_scaleBinom's scaling counts them along its first crossproduct pass and leaves them there, bed_counts / bed_MAF
do likewise, and every later solve whose variants are all known derives centre / scale from them before its first
launch — no pass counts, the plain kernels run from the start.  Integer counts feed the same arithmetic, so every
comparison here is an equality.  BSN_NO_STATS_CACHE=1 is the behaviour without the cache."""
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("d", "u", "v", "center", "scale")


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def same(a, b, what=""):
    for f in FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg="%s %s" % (what, f))
    assert (a["niter"], a["nops"]) == (b["niter"], b["nops"]), what


def served(r):
    return r["fused_stats"] and r["n_cprod_stats"] == 0


def counted(r):
    return r["fused_stats"] and r["n_cprod_stats"] >= 1


def kernels(ba, gb):
    import ctypes as C
    from bigsnpr_amd import _lib
    buf = C.create_string_buffer(8192)
    _lib.check(_lib.load().bsn_bed_streaming_kernels(gb.handle, buf, 8192))
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines() if "=" in line)


def one_plane(name):
    """k_cprod<NB, NPLANE, ...>: NPLANE = 1; k_prod<NB, CONTIG, RAWP, HASQ, ...> and k_prodT<NB, HASQ, ...>: HASQ = false"""
    family, args = name.split("<", 1)
    args = [x.strip() for x in args.split(",")]
    if family.endswith("k_cprod"):
        return args[1] == "1"
    if family.endswith("k_prodT"):
        return args[1] == "false"
    assert family.endswith("k_prod"), name
    return args[3] == "false"


@pytest.mark.parametrize("shape", [(1500, 2600), (640, 270000)])
def test_second_solve_is_served_and_identical(ba, monkeypatch, shape):
    """1 % missing; the larger shape has a warm start on the leading variants, whose launches must not count either"""
    n, m = shape
    gb = ba.bed.synthetic(n, m, seed=17)
    first = ba.bed_randomSVD(gb, k=8)
    second = ba.bed_randomSVD(gb, k=8)
    assert counted(first) and served(second)
    assert first["n_cprod_stats"] == 1       # (warm-start launches are filed under their own kind)
    assert second["n_cprod"] + second["n_wide_cprod"] == first["n_cprod"] + first["n_wide_cprod"] + 1
    assert second["warm_launches"] == first["warm_launches"] and (first["warm_launches"] > 0) == (m >= 262144)
    same(first, second, "second solve")
    monkeypatch.setenv("BSN_NO_STATS_CACHE", "1")
    off = ba.bed_randomSVD(gb, k=8)
    fresh = ba.bed_randomSVD(ba.bed.synthetic(n, m, seed=17), k=8)
    monkeypatch.delenv("BSN_NO_STATS_CACHE")
    assert counted(off) and counted(fresh)
    same(first, off, "switch off")
    same(first, fresh, "fresh handle, switch off")
    assert served(ba.bed_randomSVD(gb, k=8))     # the switch did not void what the handle knows


@pytest.mark.parametrize("compact", [True, False])
def test_column_subsets_are_served_from_the_handle(ba, monkeypatch, compact):
    """the bed_autoSVD loop: all samples, a shrinking sorted ind_col — on the compacted copy and through gather lists"""
    n, m, k = 2000, 30000, 6
    monkeypatch.setenv("BSN_COMPACT_MIN_BYTES", "0")
    if not compact:
        monkeypatch.setenv("BSN_NO_COMPACT", "1")
    rng = np.random.default_rng(5)
    gb = ba.bed.synthetic(n, m, seed=23)
    assert counted(ba.bed_randomSVD(gb, k=k))
    for t in range(3):
        ic = np.sort(rng.choice(m, 20000 - 4000 * t, replace=False))
        r = ba.bed_randomSVD(gb, ind_col=ic, k=k)
        assert served(r) and r["compacted"] == compact
        ref = ba.bed_randomSVD(ba.bed.synthetic(n, m, seed=23), ind_col=ic, k=k)
        assert counted(ref) and ref["compacted"] == compact
        same(r, ref, "list %d" % t)
    # some variants not known yet: counted as ever, and known afterwards
    gb2 = ba.bed.synthetic(n, m, seed=23)
    half = np.arange(0, m // 2)
    assert counted(ba.bed_randomSVD(gb2, ind_col=half, k=k))
    ic = np.sort(rng.choice(m, 15000, replace=False))
    r = ba.bed_randomSVD(gb2, ind_col=ic, k=k)
    assert counted(r)
    same(r, ba.bed_randomSVD(ba.bed.synthetic(n, m, seed=23), ind_col=ic, k=k), "partly known")
    again = ba.bed_randomSVD(gb2, ind_col=ic[::2].copy(), k=k)
    assert served(again)
    same(again, ba.bed_randomSVD(ba.bed.synthetic(n, m, seed=23), ind_col=ic[::2].copy(), k=k), "subset of a list")
    assert served(ba.bed_randomSVD(gb2, ind_col=half[100:9000], k=k))


def test_row_subsets_and_streamed_handles_are_not_served(ba, orc, tmp_path, monkeypatch):
    n, m, k = 1200, 2100, 5
    ob = orc.fake_bed(n, m, seed=31)
    base = str(tmp_path / "sc")
    with open(base + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(ob.payload.tobytes())
    open(base + ".fam", "w").write("".join("f%d i%d 0 0 0 -9\n" % (i, i) for i in range(n)))
    open(base + ".bim", "w").write("".join("1 s%d 0 %d A C\n" % (j, j + 1) for j in range(m)))
    gb = ba.bed(base + ".bed")
    assert counted(ba.bed_randomSVD(gb, k=k))
    ir = np.sort(np.random.default_rng(1).choice(n, 900, replace=False))
    a = ba.bed_randomSVD(gb, ind_row=ir, k=k)
    assert not a["fused_stats"]
    for compact_min in (None, "0"):        # ... nor on the compacted copy of the selected samples
        if compact_min is not None:
            monkeypatch.setenv("BSN_COMPACT_MIN_BYTES", compact_min)
        ic = np.arange(0, m, 2)
        b1 = ba.bed_randomSVD(gb, ind_row=ir, ind_col=ic, k=k)
        b2 = ba.bed_randomSVD(gb, ind_row=ir, ind_col=ic, k=k)
        assert b1["compacted"] == (compact_min is not None) and not served(b1) and not served(b2)
        monkeypatch.setenv("BSN_NO_STATS_CACHE", "1")
        same(b2, ba.bed_randomSVD(gb, ind_row=ir, ind_col=ic, k=k), "rows and columns")
        monkeypatch.delenv("BSN_NO_STATS_CACHE")
    monkeypatch.delenv("BSN_COMPACT_MIN_BYTES")
    monkeypatch.setenv("BSN_NO_STATS_CACHE", "1")
    same(a, ba.bed_randomSVD(gb, ind_row=ir, k=k), "row subset")
    monkeypatch.delenv("BSN_NO_STATS_CACHE")
    pitch = (n + 3) // 4 + 255 & ~255
    monkeypatch.setenv("BSN_IMAGE_BUDGET", str(600 * pitch))
    ooc = ba.bed(base + ".bed")
    monkeypatch.delenv("BSN_IMAGE_BUDGET")
    assert ooc.streamed
    s1, s2 = ba.bed_randomSVD(ooc, k=k), ba.bed_randomSVD(ooc, k=k)
    assert s1["out_of_core"] and counted(s1) and counted(s2)
    monkeypatch.setenv("BSN_NO_STATS_CACHE", "1")
    same(s2, ba.bed_randomSVD(ooc, k=k), "streamed handle")


def test_new_bytes_in_a_sub_image_are_counted_again(ba, monkeypatch):
    """The entries that void remembered counts and that the Python layer reaches on a live handle are the in-place
    re-gather of the compacted copy and the slab uploads of a streamed handle (never served: previous test).  After the
    copy has been overwritten by another selection, variants the handle does not know are counted again, the known ones
    are served, and both equal a fresh handle."""
    n, m, k = 2000, 30000, 6
    monkeypatch.setenv("BSN_COMPACT_MIN_BYTES", "0")
    rng = np.random.default_rng(9)
    gb = ba.bed.synthetic(n, m, seed=29)
    la = np.sort(rng.choice(m // 2, 9000, replace=False))
    lb = np.sort(m // 2 + rng.choice(m // 2, 8000, replace=False))          # disjoint from la, fits la's allocation
    lc = np.sort(np.r_[la[::3], lb[::3]])
    for ic, want in ((la, counted), (la, served), (lb, counted), (la[::2].copy(), served), (lc, served), (lb, served)):
        r = ba.bed_randomSVD(gb, ind_col=ic, k=k)
        assert r["compacted"] and want(r)
        same(r, ba.bed_randomSVD(ba.bed.synthetic(n, m, seed=29), ind_col=ic, k=k), "list of %d" % ic.size)
    gb.release_workspace()                                                   # frees the cache with the rest
    r = ba.bed_randomSVD(gb, ind_col=la, k=k)
    assert counted(r)


def test_complete_data_runs_one_plane_kernels_from_the_first_launch(ba):
    n, m = 640, 270000                       # (enough variants for a warm start on the leading sixteenth)
    gb = ba.bed.from_payload(ba.bed.synthetic(n, m, seed=41, na16=0).download(), n, m)    # nothing known about missing values
    first = ba.bed_randomSVD(gb, k=8)
    k1 = kernels(ba, gb)
    assert counted(first) and "cprod_stats" in k1
    second = ba.bed_randomSVD(gb, k=8)
    k2 = kernels(ba, gb)
    assert served(second) and "cprod_stats" not in k2 and k2
    assert "warm" in k2 and "cprod" in k2 and "prod" in k2
    for kind, name in k2.items():
        assert one_plane(name), (kind, name)
    same(first, second, "complete data")


def test_counts_and_solves_share_one_cache(ba, orc, monkeypatch):
    n, m, k = 1100, 3000, 5
    ob = orc.fake_bed(n, m, seed=37)
    want = orc.bed_col_counts(ob)
    rng = np.random.default_rng(3)
    ic = rng.permutation(m)[:1200]
    # a solve, then the counts
    gb = ba.bed.from_payload(ob.payload, n, m)
    ref = ba.bed_randomSVD(gb, k=k)
    assert counted(ref)
    np.testing.assert_array_equal(ba.bed_counts(gb), want)
    np.testing.assert_array_equal(ba.bed_counts(gb, None, ic), want[:, ic])
    np.testing.assert_array_equal(ba.bed_MAF(gb)["maf"], orc.bed_MAF(ob)["maf"])
    # the counts, then a solve
    gb2 = ba.bed.from_payload(ob.payload, n, m)
    np.testing.assert_array_equal(ba.bed_counts(gb2, None, np.arange(500, m)), want[:, 500:])
    r = ba.bed_randomSVD(gb2, ind_col=np.arange(600, m), k=k)
    assert served(r)
    monkeypatch.setenv("BSN_NO_STATS_CACHE", "1")
    same(r, ba.bed_randomSVD(ba.bed.from_payload(ob.payload, n, m), ind_col=np.arange(600, m), k=k), "after bed_counts")
    monkeypatch.delenv("BSN_NO_STATS_CACHE")
    assert counted(ba.bed_randomSVD(gb2, k=k))                  # variants 0 .. 499 were not known
    np.testing.assert_array_equal(ba.bed_counts(gb2), want)
    assert served(ba.bed_randomSVD(gb2, k=k))
    sc = orc.bed_scaleBinom(ob)
    np.testing.assert_array_equal(ref["center"], sc["center"])
    np.testing.assert_array_equal(ref["scale"], sc["scale"])


def test_served_solve_still_warns_of_mostly_missing_variants(ba, orc):
    n, m = 400, 300
    ob = orc.fake_bed(n, m, seed=9)
    payload = ob.payload.copy().reshape(m, -1)
    payload[7, : payload.shape[1] * 3 // 4] = 0x55        # code 01 = missing for 3/4 of variant 7
    payload[200, : payload.shape[1] * 2 // 3] = 0x55
    gb = ba.bed.from_payload(payload.reshape(-1), n, m)
    results = []
    for _ in range(2):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            results.append(ba.bed_randomSVD(gb, k=3))
        assert any("2 variants have >50% missing values." in str(x.message) for x in w)
    assert counted(results[0]) and served(results[1])
    same(results[0], results[1], "mostly missing variants")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r = ba.bed_randomSVD(gb, ind_col=np.arange(100, 300), k=3)
    assert served(r) and any("1 variants have >50% missing values." in str(x.message) for x in w)
