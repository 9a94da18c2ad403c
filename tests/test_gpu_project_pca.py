"""The OADP projection on the device and bed_projectPCA (bigsnpr_amd/project.py, prs.py over csrc/project.hip and
csrc/oadp_step.hpp).

* bsn_pca_oadp_proj equals the CPU statement of the same header (tests/native/oadp_ref.cpp) at rtol = 1e-9,
  atol = 1e-9 d[0] — the tolerance of the project's OADP comparisons: one sample, one workgroup's worth of samples plus
  3, and 1 003 samples (hundreds of workgroups) for each of the four lane mappings; K on both sides of every boundary of
  the lane mapping (K + 1 <= 8, 16, 32, else a whole wave) and at the cap; the edge rows (a zero sample, |y|^2 = |l|^2,
  |y|^2 just below |l|^2, |y|^2 > 9 d_1^2, a NaN row) first and last in the batch; two equal singular values.
* bsn_bed_project_pca equals prod_and_rowSumsSq followed by the CPU statement: all rows, a row subset, a column subset
  with negative scales.
* the assertion of tests/testthat/test-2-pca-project.R:69-80 of the reference: bed_projectPCA of a file on itself equals
  bed_autoSVD + bed_projectSelfPCA, at the reference's 1e-6 (all.equal's mean relative difference).
* allele handling end to end: a target with reversed, strand-flipped and ambiguous variants projects like the
  unmodified genotypes; the ambiguous variants are not in `subset`.
* oadp = "device" equals oadp = "host" on bed_projectSelfPCA and snp_projectSelfPCA (NaN rows included).
* the argument errors carry their messages."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import oadp_inputs as inp  # noqa: E402
import oadp_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = ref.max_k()
KS = (1, 2, 7, 8, 15, 16, 20, 31, 32, CAP)      # 7 | 8, 15 | 16, 31 | 32: the boundaries of the lane mapping


def group_width(K):
    """lanes per sample (project.hip)"""
    return 8 if K + 1 <= 8 else 16 if K + 1 <= 16 else 32 if K + 1 <= 32 else 64


def per_workgroup(K):
    return 64 // group_width(K)


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def _close(got, want, d, nan_rows=None):
    if nan_rows is not None:
        assert np.isnan(got[nan_rows]).all() and np.isfinite(got[~nan_rows]).all()
        got, want = got[~nan_rows], want[~nan_rows]
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9 * np.max(d))


def _kernel_case(ba, K, n):
    d = inp.sval(K, seed=K, equal_pair=True)
    XV, X_norm, rows = inp.batch(n, d, seed=100 + K)
    got = ba.pca_OADP_proj_device(XV, X_norm, d)
    want = ref.proj(XV, X_norm, d)
    assert got.shape == (n, K)
    _close(got, want, d, ~inp.finite_rows(n, rows))
    return rows


@pytest.mark.parametrize("K", KS)
def test_kernel_equals_the_cpu_statement_one_sample(ba, K):
    _kernel_case(ba, K, 1)


@pytest.mark.parametrize("K", KS)
def test_kernel_equals_the_cpu_statement_past_one_workgroup(ba, K):
    rows = _kernel_case(ba, K, per_workgroup(K) + 3)
    if per_workgroup(K) + 3 >= 2 * len(inp.EDGE_KINDS):
        assert list(rows.values()).count("nan") == 2        # the edge rows sit first AND last


@pytest.mark.parametrize("K", (1, 8, 20, 32))       # one K per lane mapping: 8, 16, 32 and 64 lanes per sample
def test_kernel_equals_the_cpu_statement_many_workgroups(ba, K):
    rows = _kernel_case(ba, K, 1003)
    assert rows[0] == rows[1002] and len(rows) == 2 * len(inp.EDGE_KINDS)


def test_kernel_distinct_singular_values_and_unsorted(ba):
    for d in (inp.sval(20, seed=3), inp.sval(6, seed=1)[::-1].copy()):
        XV, X_norm, rows = inp.batch(37, d, seed=9)
        _close(ba.pca_OADP_proj_device(XV, X_norm, d), ref.proj(XV, X_norm, d), d, ~inp.finite_rows(37, rows))


def test_argument_errors(ba):
    d = inp.sval(4, seed=3)
    XV, X_norm, _ = inp.batch(3, d, seed=1)
    for bad in (0.0, -3.0, np.nan, np.inf):
        d2 = d.copy()
        d2[2] = bad
        with pytest.raises(ba.BsnError, match="singular values must be finite and positive"):
            ba.pca_OADP_proj_device(XV, X_norm, d2)
    big = inp.sval(CAP + 1, seed=0)
    XVb, Xnb, _ = inp.batch(2, big, seed=0)
    with pytest.raises(ba.BsnError, match="more than %d singular values" % CAP):
        ba.pca_OADP_proj_device(XVb, Xnb, big)
    with pytest.raises(ValueError, match="Incompatibility between dimensions"):
        ba.pca_OADP_proj_device(XV, X_norm[:2], d)
    assert ba.pca_OADP_proj_device(XV[:0], X_norm[:0], d).shape == (0, 4)


# ---- on example.bed -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example(ba, golden_dir):
    return ba.bed(os.path.join(golden_dir, "example.bed"))


@pytest.fixture(scope="module")
def split(example):
    rng = np.random.default_rng(11)
    train = np.sort(rng.choice(example.nrow, 400, replace=False))
    test = np.setdiff1d(np.arange(example.nrow), train)
    return train, test


@pytest.fixture(scope="module")
def auto_svd(ba, example, split):
    return ba.bed_autoSVD(example, ind_row=split[0], roll_size=10, thr_r2=0.8, verbose=False)


def test_fused_call_equals_its_parts(ba, example, split):
    train, test = split
    svd = ba.bed_randomSVD(example, ind_row=train, k=5)
    m = example.ncol
    rng = np.random.default_rng(2)
    some_rows = rng.permutation(test)[:77]
    some_cols = np.sort(rng.choice(m, 1201, replace=False))
    sign = np.where(rng.random(some_cols.size) < 0.3, -1.0, 1.0)
    cases = ((None, np.arange(m), svd["center"], svd["scale"], svd["v"]),
             (some_rows, np.arange(m), svd["center"], svd["scale"], svd["v"]),
             (test, some_cols, (svd["center"][some_cols] - 1.0) * sign + 1.0, svd["scale"][some_cols] * sign,
              svd["v"][some_cols]))
    for ir, ic, center, scale, V in cases:
        XV, rs, oadp = ba.project_pca(example, ir, ic, center, scale, V, svd["d"])
        XV0, rs0 = ba.prod_and_rowSumsSq(example, ir, ic, center, scale, V)
        assert np.array_equal(XV, XV0) and np.array_equal(rs, rs0)
        _close(oadp, ref.proj(XV0, rs0, svd["d"]), svd["d"])
        assert np.isfinite(oadp).all()
    assert (cases[2][3] < 0).sum() > 100


def _mean_rel_diff(target, current):
    """all.equal(): mean(abs(target - current)) / mean(abs(target))"""
    target, current = np.asarray(target, dtype=np.float64), np.asarray(current, dtype=np.float64)
    return np.abs(target - current).sum() / np.abs(target).sum()


def test_project_pca_of_a_file_on_itself_equals_autosvd_and_self_projection(ba, example, split, auto_svd):
    """tests/testthat/test-2-pca-project.R:69-80"""
    train, test = split
    proj2 = ba.bed_projectPCA(example, example, ind_row_new=test, ind_row_ref=train, strand_flip=False, roll_size=10,
                              thr_r2=0.8, verbose=False)
    proj3 = ba.bed_projectSelfPCA(auto_svd, example, ind_row=test, oadp="device")
    assert sorted(proj2) == ["OADP_proj", "obj_svd_ref", "simple_proj"]
    assert np.array_equal(proj2["obj_svd_ref"]["subset"], proj3["obj_svd_ref"]["subset"])
    for key in ("d", "u", "v", "center", "scale"):
        assert _mean_rel_diff(proj3["obj_svd_ref"][key], proj2["obj_svd_ref"][key]) < 1e-6, key
    for key in ("simple_proj", "OADP_proj"):
        assert proj2[key].shape == (test.size, 10)
        assert _mean_rel_diff(proj3[key], proj2[key]) < 1e-6, key


def test_alleles_reversed_flipped_and_ambiguous_end_to_end(ba, golden_dir, tmp_path, split):
    train, test = split
    big = ba.snp_readBed(os.path.join(golden_dir, "example.bed"))
    g = big["bytes"]
    m = g.shape[1]
    assert (g <= 2).all()
    rng = np.random.default_rng(5)
    kind = rng.choice(4, size=m, p=(0.55, 0.2, 0.2, 0.05))      # 0 as is, 1 reversed, 2 strand-flipped, 3 ambiguous
    pairs = np.array([("A", "C"), ("A", "G"), ("C", "T"), ("G", "T"), ("C", "A"), ("T", "G")])
    a = pairs[rng.integers(0, len(pairs), size=m)]
    a[kind == 3] = np.array([("A", "T"), ("C", "G")])[rng.integers(0, 2, size=(kind == 3).sum())]
    map_ref = dict(big["map"], allele1=list(a[:, 0]), allele2=list(a[:, 1]))
    flip = {"A": "T", "C": "G", "G": "C", "T": "A"}
    b = a.copy()
    b[kind == 1] = a[kind == 1][:, ::-1]
    b[kind == 2] = np.vectorize(flip.get)(a[kind == 2])
    g_new = g.copy()
    g_new[:, kind == 1] = 2 - g[:, kind == 1]
    map_new = dict(big["map"], allele1=list(b[:, 0]), allele2=list(b[:, 1]))
    ref_bed = ba.bed(ba.snp_writeBed(dict(genotypes=ba.FBM_code256(g), fam=big["fam"], map=map_ref), str(tmp_path / "ref.bed")))
    new_bed = ba.bed(ba.snp_writeBed(dict(genotypes=ba.FBM_code256(g_new), fam=big["fam"], map=map_new),
                                     str(tmp_path / "new.bed")))
    args = dict(ind_row_new=test, ind_row_ref=train, roll_size=10, thr_r2=0.8, verbose=False)
    got = ba.bed_projectPCA(ref_bed, new_bed, **args)
    want = ba.bed_projectPCA(ref_bed, ref_bed, **args)
    subset = got["obj_svd_ref"]["subset"]
    assert np.array_equal(subset, want["obj_svd_ref"]["subset"])
    assert not np.isin(np.nonzero(kind == 3)[0], subset).any() and (kind == 3).sum() > 50
    assert (kind[subset] == 1).sum() > 100 and (kind[subset] == 2).sum() > 100
    for key in ("simple_proj", "OADP_proj"):
        assert _mean_rel_diff(want[key], got[key]) < 1e-6, key
    # and without the allele handling the reversed variants would have shown
    plain = ba.bed_projectSelfPCA(got["obj_svd_ref"], new_bed, ind_row=test, oadp="device")
    assert _mean_rel_diff(want["simple_proj"], plain["simple_proj"]) > 1e-2


def test_build_mismatch_errors(ba, example):
    with pytest.raises(ValueError, match="Please provide path to liftOver executable."):
        ba.bed_projectPCA(example, example, build_new="hg38", verbose=False)
    with pytest.raises(NotImplementedError, match="external executable, not emulated"):
        ba.bed_projectPCA(example, example, build_new="hg38", liftOver="./liftOver", verbose=False)
    with pytest.raises(ValueError, match="Not enough variants have been matched."):
        ba.bed_projectPCA(example, example, verbose=False)      # example.bim is A/T throughout: all ambiguous


def test_device_oadp_equals_host_oadp_on_both_self_projections(ba, orc, golden_dir, example, split, auto_svd, missing_bed):
    train, test = split
    host = ba.bed_projectSelfPCA(auto_svd, example, ind_row=test)
    dev = ba.bed_projectSelfPCA(auto_svd, example, ind_row=test, oadp="device")
    assert np.array_equal(host["simple_proj"], dev["simple_proj"]) and np.array_equal(host["X_norm"], dev["X_norm"])
    _close(dev["OADP_proj"], host["OADP_proj"], auto_svd["d"])

    # an FBM with missing codes: the affected rows are NaN in both
    gm = ba.bed(os.path.join(golden_dir, "example-missing.bed"))
    Gm = ba.FBM_code256(orc.fbm_from_bed(missing_bed).bytes)
    sc = ba.bed_scaleBinom(gm)
    ic = np.nonzero(sc["scale"] > 0)[0][:60]
    rng = np.random.default_rng(6)
    V = np.linalg.qr(rng.normal(size=(ic.size, 3)))[0]
    svd = dict(v=V, d=np.array([30.0, 20.0, 10.0]), center=sc["center"][ic], scale=sc["scale"][ic])
    rows = np.arange(gm.nrow)
    h = ba.snp_projectSelfPCA(svd, Gm, ind_row=rows, ind_col=ic)
    dv = ba.snp_projectSelfPCA(svd, Gm, ind_row=rows, ind_col=ic, oadp="device")
    nan_rows = np.isnan(h["OADP_proj"]).any(axis=1)
    assert 0 < nan_rows.sum() < rows.size
    assert np.array_equal(h["simple_proj"], dv["simple_proj"], equal_nan=True)
    _close(dv["OADP_proj"], h["OADP_proj"], svd["d"], nan_rows)
    with pytest.raises(ValueError, match="'oadp' should be"):
        ba.bed_projectSelfPCA(auto_svd, example, ind_row=test, oadp="gpu")
