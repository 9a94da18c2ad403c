"""Per-group genotype counts, snp_fst and snp_MAX3 on the device (bigsnpr_amd/popstat.py over csrc/popstat.hip and
counts_grouped of csrc/matvec.hip).

* bed_counts_by_group equals a numpy count over the decoded genotypes: one sample / a ragged tail past the 512-sample
  chunk / a third chunk; one variant / more than the 256 of a workgroup; 1, 2, 3, 16, 17 and 33 groups (one column block,
  two, a second launch); labels -1, an empty group, a file row under two groups, unsorted rows with repeats, one row 130
  times (the four-digit panel); on the streaming-layout copy, on an out-of-core handle, on an FBM.code256; and equals
  bed_counts group by group.
* bed_fst, snp_fst(bed_MAF_by_group(...)) and the CPU statement (tests/native/popstat_ref.cpp) are bit-identical, per
  variant and overall.
* snp_MAX3 reproduces the nine published statistics of Zheng et al. 2012 and equals the CPU statement bit for bit.
* the argument errors carry their messages."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

import popstat_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 3, 16, 17, 33)
NA16 = 1966   # 3 % of 65536


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def numpy_counts(Gm, ir, labels, G, ic):
    """(G, 4, m) from the decoded n x m matrix (3 = missing)"""
    out = np.zeros((G, 4, ic.size), dtype=np.int32)
    sub = Gm[np.ix_(ir, ic)]
    for g in range(G):
        rows = sub[labels == g]
        for c in range(4):
            out[g, c] = (rows == c).sum(axis=0)
    return out


def selection(rng, n, G, heavy):
    """rows (unsorted, with repeats; `heavy`: one of them 130 times under one group) and their labels: -1 for some, an
    empty group where there are three or more, one file row under two groups where there are two or more"""
    k = max(4, n + n // 3)
    ir = rng.integers(0, n, size=k)
    empty = G - 1 if G >= 3 else -5
    pool = np.array([g for g in range(-1, G) if g != empty])
    lab = rng.choice(pool, size=k)
    lab[0] = -1
    if G >= 2:
        ir[1] = ir[2] = n // 2
        lab[1], lab[2] = 0, 1
    if heavy:
        ir = np.concatenate([ir, np.full(130, n - 1)])
        lab = np.concatenate([lab, np.full(130, 0)])
        p = rng.permutation(ir.size)
        ir, lab = ir[p], lab[p]
    return ir.astype(np.int64), lab.astype(np.int64), empty


def payload_handle(ba, orc, n, m, seed):
    ob = orc.fake_bed(n, m, seed=seed, na16=NA16)
    return ob, ba.bed.from_payload(ob.payload, n, m), np.ascontiguousarray(orc.read_bed(ob, na_val=3))


# ---- counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 517, 1100])
@pytest.mark.parametrize("m", [1, 300])
def test_counts_by_group_equal_numpy(ba, orc, n, m):
    ob, gb, Gm = payload_handle(ba, orc, n, m, seed=n + m)
    if n * m > 1000:
        assert 0.02 < (Gm == 3).mean() < 0.04
    rng = np.random.default_rng(n * 7 + m)
    contig = np.arange(m) if m == 1 else np.arange(37, 37 + 201)                        # from an odd offset
    ragged = np.array([0, 0, 0]) if m == 1 else rng.integers(0, m, size=283)            # unsorted, with repeats
    for G in GROUPS:
        for heavy, ic in ((False, contig), (True, ragged)):
            ir, lab, empty = selection(rng, n, G, heavy)
            got = ba.bed_counts_by_group(gb, lab, ind_row=ir, ind_col=ic, n_groups=G)
            assert got.shape == (G, 4, ic.size) and got.dtype == np.int32
            want = numpy_counts(Gm, ir, lab, G, ic)
            np.testing.assert_array_equal(got, want, err_msg="n=%d m=%d G=%d heavy=%s" % (n, m, G, heavy))
            if empty >= 0:
                assert not got[empty].any()
            if heavy:
                assert got[0].sum(axis=0).min() >= 130
    # all rows in file order, every variant
    lab = rng.integers(-1, 3, size=n)
    np.testing.assert_array_equal(ba.bed_counts_by_group(gb, lab, n_groups=3), numpy_counts(Gm, np.arange(n), lab, 3, np.arange(m)))
    gb.close()


def test_counts_on_the_tiled_copy_streamed_handle_and_fbm(ba, orc, tmp_path, monkeypatch):
    n, m = 1100, 300
    ob, gb, Gm = payload_handle(ba, orc, n, m, seed=77)
    rng = np.random.default_rng(5)
    calls = []
    for G, heavy in ((3, False), (17, False), (5, True), (33, False)):
        ir, lab, _ = selection(rng, n, G, heavy)
        for ic in (None, rng.integers(0, m, size=150), np.arange(64, 64 + 130)):
            calls.append((G, ir, lab, ic))

    def run(obj):
        return [ba.bed_counts_by_group(obj, lab, ind_row=ir, ind_col=ic, n_groups=G) for G, ir, lab, ic in calls]
    plain = run(gb)
    for (G, ir, lab, ic), got in zip(calls, plain):
        np.testing.assert_array_equal(got, numpy_counts(Gm, ir, lab, G, np.arange(m) if ic is None else ic))
    # the streaming-layout copy serves the 64-aligned contiguous selections
    assert gb.tile() is True
    for a, b in zip(plain, run(gb)):
        np.testing.assert_array_equal(a, b)
    gb.close()
    # an out-of-core handle: slabs of 64 variants
    path = str(tmp_path / "grp.bed")
    ob.raw.tofile(path)
    (tmp_path / "grp.bim").write_text("".join("1\tsnp%d\t0\t%d\tA\tT\n" % (j, j + 1) for j in range(m)))
    (tmp_path / "grp.fam").write_text("".join("f%d i%d 0 0 0 -9\n" % (i, i) for i in range(n)))
    pitch = (n + 3) // 4 + 255 & ~255
    monkeypatch.setenv("BSN_IMAGE_BUDGET", str(130 * pitch))
    ooc = ba.bed(path)
    monkeypatch.delenv("BSN_IMAGE_BUDGET")
    assert ooc.streamed
    for a, b in zip(plain, run(ooc)):
        np.testing.assert_array_equal(a, b)
    ooc.close()
    # an FBM.code256 with CODE_012
    fbm = ba.FBM_code256(Gm.astype(np.uint8), ba.CODE_012)
    for a, b in zip(plain, run(fbm)):
        np.testing.assert_array_equal(a, b)


def test_counts_by_group_equal_bed_counts(ba, golden_dir):
    gb = ba.bed(os.path.join(golden_dir, "example-missing.bed"))
    n, m = gb.nrow, gb.ncol
    rng = np.random.default_rng(11)
    lab = rng.integers(-1, 4, size=n)
    ir = rng.permutation(n)
    before = ba.bed_counts(gb, ind_row=np.arange(0, n, 2))
    got = ba.bed_counts_by_group(gb, lab, ind_row=ir)
    assert got.shape == (4, 4, m)
    for g in range(4):
        np.testing.assert_array_equal(got[g], ba.bed_counts(gb, ind_row=ir[lab == g]))
    mafs = ba.bed_MAF_by_group(gb, lab, ind_row=ir)
    for g in range(4):
        one = ba.bed_MAF(gb, ind_row=ir[lab == g])
        for f in ("ac", "mac", "af", "maf", "N"):
            np.testing.assert_array_equal(mafs[g][f], one[f])
    np.testing.assert_array_equal(ba.bed_counts(gb, ind_row=np.arange(0, n, 2)), before)
    gb.close()


# ---- Fst -------------------------------------------------------------------------------------------------------------------------
def check_fst(ba, obj, lab, G, min_maf, ir=None, ic=None):
    """the three routes, bit for bit; returns the twin's result"""
    mafs = ba.bed_MAF_by_group(obj, lab, ind_row=ir, ind_col=ic, n_groups=G)
    af, N = np.stack([d["af"] for d in mafs]), np.stack([d["N"] for d in mafs]).astype(np.float64)
    t = ref.fst(af, N, min_maf)
    per = ba.bed_fst(obj, lab, ind_row=ir, ind_col=ic, min_maf=min_maf, n_groups=G)
    np.testing.assert_array_equal(per, t["fst"])
    np.testing.assert_array_equal(ba.snp_fst(mafs, min_maf=min_maf), t["fst"])
    assert np.array_equal(np.isnan(per), ~t["keep"])
    ov = ba.bed_fst(obj, lab, ind_row=ir, ind_col=ic, min_maf=min_maf, overall=True, n_groups=G)
    ov2 = ba.snp_fst(mafs, min_maf=min_maf, overall=True)
    assert isinstance(ov, float) and ov == ov2 == t["overall"][0], (ov, ov2, t["overall"])
    return t


def test_fst_example_bed(ba, golden_dir):
    gb = ba.bed(os.path.join(golden_dir, "example.bed"))
    pop = np.repeat([0, 1, 2], [143, 167, 207])
    t = check_fst(ba, gb, pop, 3, 0.0)
    assert t["keep"].all() and 0.0236 <= t["overall"][0] <= 0.0238
    for a, b in ((0, 1), (0, 2), (2, 1)):
        lab = np.full(517, -1)
        lab[pop == a], lab[pop == b] = 0, 1
        check_fst(ba, gb, lab, 2, 0.0)
    # the reference's way, one bed_MAF per population
    lst = [ba.bed_MAF(gb, ind_row=np.nonzero(pop == p)[0]) for p in range(3)]
    assert ba.snp_fst(lst, overall=True) == t["overall"][0]
    np.testing.assert_array_equal(ba.snp_fst(lst), t["fst"])
    gb.close()


def test_fst_example_missing(ba, golden_dir):
    gb = ba.bed(os.path.join(golden_dir, "example-missing.bed"))
    lab = np.repeat([0, 1], [100, 100])
    for min_maf in (0.0, 0.05):
        check_fst(ba, gb, lab, 2, min_maf)
    gb.close()


@pytest.mark.parametrize("m", [257, 1000])
def test_fst_synthetic_with_monomorphic_variants(ba, m):
    rng = np.random.default_rng(m)
    n = 330
    f = rng.uniform(0.01, 0.5, size=m)
    raw = rng.binomial(2, f[None, :], size=(n, m)).astype(np.uint8)
    raw[rng.random((n, m)) < 0.03] = 3
    mono = np.arange(3, m, 9)
    raw[:, mono] = 0
    raw[:, 5] = 3                                  # a variant without any call
    raw[:110, 6] = 3                               # all NA in the first group
    fbm = ba.FBM_code256(raw, ba.CODE_012)
    lab = np.repeat([0, 1, 2], 110)
    t = check_fst(ba, fbm, lab, 3, 0.05)
    assert not t["keep"][mono].any() and not t["keep"][5] and not t["keep"][6] and 0 < t["keep"].sum() < m - mono.size
    t0 = check_fst(ba, fbm, lab, 3, 0.0)
    assert t0["keep"].sum() > t["keep"].sum()
    # a shuffled subset of rows, unsorted variants
    ir, ic = rng.permutation(n)[:250], rng.permutation(m)[: m // 2]
    check_fst(ba, fbm, lab[ir], 3, 0.05, ir=ir, ic=ic)


# ---- MAX3 ------------------------------------------------------------------------------------------------------------------------
def test_max3_published_table(ba, golden_dir):
    """the image of tests/testthat/test-4-MAX3.R:31-51: cases first, controls second, each variant padded with NA to the
    largest table (1172 cases + 1157 controls = 2329 samples, 9 variants)"""
    with open(os.path.join(golden_dir, "max3_zheng2012.json")) as fh:
        z = json.load(fh)
    cases, controls, want = np.array(z["cases"]), np.array(z["controls"]), np.array(z["sqrt_score"])
    n_ca, n_co = cases.sum(axis=1).max(), controls.sum(axis=1).max()
    assert (n_ca, n_co) == (1172, 1157)
    rng = np.random.default_rng(1)
    raw = np.full((n_ca + n_co, 9), 3, dtype=np.uint8)
    for j in range(9):
        ca = np.concatenate([np.repeat([0, 1, 2], cases[j]), np.full(n_ca - cases[j].sum(), 3)])
        co = np.concatenate([np.repeat([0, 1, 2], controls[j]), np.full(n_co - controls[j].sum(), 3)])
        raw[:, j] = np.concatenate([rng.permutation(ca), rng.permutation(co)])
    y01 = np.repeat([1, 0], [n_ca, n_co])
    fbm = ba.FBM_code256(raw, ba.CODE_012)
    res = ba.snp_MAX3(fbm, y01)
    got = np.sqrt(res["score"])
    assert np.array_equal(np.round(got, 3), want), got
    for val in ((0, 0.5, 1), (0.5,), np.linspace(0, 1, 33)):
        np.testing.assert_array_equal(ba.snp_MAX3(fbm, y01, val=val)["score"], ref.max3(cases.T, controls.T, val))
    from scipy.stats import rankdata
    np.testing.assert_array_equal(rankdata(res["score"]), rankdata(-res["predict"]()))


def test_max3_random_subset(ba, orc):
    n, m = 700, 300
    ob, gb, Gm = payload_handle(ba, orc, n, m, seed=3)
    rng = np.random.default_rng(9)
    ind = rng.permutation(n)[:450]
    y01 = rng.integers(0, 2, size=450)
    y01[:20] = 1
    for val in ((0, 0.5, 1), (0.5,), np.linspace(0, 1, 33)):
        res = ba.snp_MAX3(gb, y01, ind_train=ind, val=val)
        ca = np.array([(Gm[ind[y01 == 1]] == c).sum(axis=0) for c in range(3)])
        co = np.array([(Gm[ind[y01 == 0]] == c).sum(axis=0) for c in range(3)])
        np.testing.assert_array_equal(res["score"], ref.max3(ca, co, val))
    from scipy.stats import rankdata
    res = ba.snp_MAX3(gb, y01, ind_train=ind)
    np.testing.assert_array_equal(rankdata(res["score"]), rankdata(-res["predict"]()))
    # cases only: every score is 0
    assert not ba.snp_MAX3(gb, np.ones(450), ind_train=ind)["score"].any()
    gb.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(ba, golden_dir):
    gb = ba.bed(os.path.join(golden_dir, "example-missing.bed"))
    n = gb.nrow
    one = ba.bed_MAF(gb)
    with pytest.raises(ba.BsnError, match="You should provide frequencies for at least 2 populations."):
        ba.snp_fst([one])
    with pytest.raises(ba.BsnError, match="You should provide frequencies for at least 2 populations."):
        ba.bed_fst(gb, np.zeros(n, dtype=int))
    with pytest.raises(ba.BsnError, match=r"Parameter 'min_maf' should be in range \[0, 0.45\]."):
        ba.snp_fst([one, one], min_maf=0.5)
    with pytest.raises(ba.BsnError, match=r"Parameter 'min_maf' should be in range \[0, 0.45\]."):
        ba.bed_fst(gb, np.arange(n) % 2, min_maf=-0.1)
    lab = np.arange(n) % 3
    with pytest.raises(ba.BsnError, match=r"label 2 of row 2 is outside -1 \.\. 1"):
        ba.bed_counts_by_group(gb, lab, n_groups=2)
    lab = lab.copy()
    lab[7] = -2
    with pytest.raises(ba.BsnError, match=r"label -2 of row 7 is outside -1 \.\. 2"):
        ba.bed_counts_by_group(gb, lab)
    with pytest.raises(ba.BsnError, match="number of groups should be at least 1"):
        ba.bed_counts_by_group(gb, np.full(n, -1))
    with pytest.raises(ValueError, match="should have the same length"):
        ba.bed_counts_by_group(gb, lab[:-1])
    y = np.arange(n) % 2
    y[5] = 2
    with pytest.raises(ba.BsnError, match=r"should hold 0 \(control\) or 1 \(case\) only; row 5 holds 2"):
        ba.snp_MAX3(gb, y)
    with pytest.raises(ba.BsnError, match="'val' should hold at least one value"):
        ba.snp_MAX3(gb, np.arange(n) % 2, val=())
    gb.close()
    rng = np.random.default_rng(0)
    dos = ba.FBM_code256(rng.integers(7, 208, size=(64, 20)).astype(np.uint8), ba.CODE_DOSAGE)
    with pytest.raises(ba.BsnError, match="bed_counts_by_group is not available for this handle: it needs a 2-bit genotype image"):
        ba.bed_counts_by_group(dos, np.arange(64) % 2)
    with pytest.raises(ba.BsnError, match="needs a 2-bit genotype image"):
        ba.snp_MAX3(dos, np.arange(64) % 2)
