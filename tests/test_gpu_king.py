"""bed_king / bed_kingQC on the device (bigsnpr_amd/csrc/king.hip) against the CPU statement over the same king_step.hpp
(tests/native/king_ref.cpp): indices and the five counts equal, the kinship bit for bit.  Shapes are built in NumPy from
fixed seeds; the pair kernel's tile edge is 64 samples and its K-step 256 variants of a 512-variant chunk, so the shapes sit
on both sides of 64 / 128 samples and of 64 / 512 / 1024 variants."""
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import king_cases as kc  # noqa: E402
import king_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (3, 63), (17, 64), (64, 65), (65, 511), (129, 512), (257, 513), (130, 1100)]


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


def handle(ba, G):
    return ba.bed.from_payload(kc.encode_payload(G), G.shape[0], G.shape[1])


def check_ms(ms, complete):
    assert len(ms) == 4 and all(np.isfinite(v) and v >= 0 for v in ms)
    assert ms[2] > 0 and ms[3] > 0
    assert (ms[1] > 0) == complete      # the per-sample totals run on the two-product path alone


@pytest.mark.parametrize("n,m", SHAPES)
def test_table_equals_twin(ba, n, m):
    G = kc.random_codes(n, m, 0.03, seed=1000 + 7 * n + m)
    b = handle(ba, G)
    got = ba.bed_king(b)
    ms = ba.king_last_ms()
    want = ref.table(G)
    kc.assert_same_table(got, want)
    assert got["KINSHIP"].size == n * (n - 1) // 2
    check_ms(ms, complete=False)
    assert ms[0] > 0                    # a fresh handle: the sample-major copy was built by this call
    if n > 128:                         # more than two tile edges: a tile pair and its transpose, rows and columns, cannot be swapped
        assert (got["HET1HOM2"] != got["HET2HOM1"]).any()


def test_complete_data_two_products(ba, monkeypatch):
    """no missing call, known to the handle: x.x and H.H are the only matrix products; same rows as the seven-product path"""
    G = kc.random_codes(130, 1100, 0.0, seed=77)
    b = handle(ba, G)
    assert ba.bed_counts(b)[3].sum() == 0
    assert int(ba.load().bsn_bed_na_known(b.handle)) == 0
    two = ba.bed_king(b)
    check_ms(ba.king_last_ms(), complete=True)
    monkeypatch.setenv("BSN_KING_GENERAL", "1")
    seven = ba.bed_king(b)
    check_ms(ba.king_last_ms(), complete=False)
    monkeypatch.delenv("BSN_KING_GENERAL")
    kc.assert_same_table(two, seven)
    kc.assert_same_table(two, ref.table(G))
    assert (two["NSNP"] == 1100).all() and (two["HET1HOM2"] != two["HET2HOM1"]).any()
    # ... also under a row list and a column list (the totals are those of the selection)
    ir, ic = np.array([129, 3, 64, 3, 70, 0, 128]), np.arange(1099, -1, -3)
    kc.assert_same_table(ba.bed_king(b, ind_row=ir, ind_col=ic), ref.table(G[np.ix_(ir, ic)]))
    check_ms(ba.king_last_ms(), complete=True)


def test_padding_nsnp(ba):
    """the pad variants of the last chunk are called homozygotes in the operand: NSNP must not count them"""
    G = kc.random_codes(65, 511, 0.0, seed=5)
    b = handle(ba, G)
    t = ba.bed_king(b)                                  # completeness not known yet: the general path
    check_ms(ba.king_last_ms(), complete=False)
    assert t["NSNP"].size == 65 * 64 // 2 and (t["NSNP"] == 511).all()
    kc.assert_same_table(t, ref.table(G))
    ba.bed_counts(b)
    t2 = ba.bed_king(b)
    check_ms(ba.king_last_ms(), complete=True)
    kc.assert_same_table(t2, t)


def test_ind_row_unsorted_with_repeat(ba):
    G = kc.random_codes(140, 700, 0.03, seed=9)
    ir = np.array([139, 5, 64, 130, 5, 0, 63, 128, 77, 1])
    assert ((G[5] == 1).sum()) > 0
    t = ba.bed_king(handle(ba, G), ind_row=ir)
    kc.assert_same_table(t, ref.table(G[ir]))
    k = int(np.flatnonzero((t["I1"] == 1) & (t["I2"] == 4))[0])      # both copies of sample 5
    assert t["KINSHIP"][k] == 0.5
    assert t["IBS0"][k] == 0 and t["HET1HOM2"][k] == 0 and t["HET2HOM1"][k] == 0
    # more rows than samples, past two tile edges
    rng = np.random.default_rng(4)
    ir = rng.integers(0, 140, size=150)
    kc.assert_same_table(ba.bed_king(handle(ba, G), ind_row=ir), ref.table(G[ir]))


def test_repeat_without_heterozygote_is_nan(ba):
    G = kc.random_codes(6, 90, 0.03, seed=10)
    G[2][G[2] == 1] = 0
    t = ba.bed_king(handle(ba, G), ind_row=np.array([2, 4, 2]))
    kc.assert_same_table(t, ref.table(G[[2, 4, 2]]))
    assert np.isnan(t["KINSHIP"][1])                                 # pair (0, 2): 0 / 0


@pytest.mark.parametrize("cols", ["strided", "unsorted"])
def test_ind_col(ba, cols):
    G = kc.random_codes(131, 1300, 0.03, seed=12)
    ic = np.arange(1, 1300, 2) if cols == "strided" else np.random.default_rng(2).permutation(1300)[:777]
    b = handle(ba, G)
    kc.assert_same_table(ba.bed_king(b, ind_col=ic), ref.table(G[:, ic]))
    ir = np.array([130, 2, 65, 2, 64])
    kc.assert_same_table(ba.bed_king(b, ind_row=ir, ind_col=ic), ref.table(G[np.ix_(ir, ic)]))
    kc.assert_same_table(ba.bed_king(b), ref.table(G))             # the handle itself is unchanged


def test_filter_rows_and_determinism(ba):
    G = kc.random_codes(150, 600, 0.03, seed=14)
    rng = np.random.default_rng(15)
    for child, (p1, p2) in {149: (3, 70), 10: (129, 5), 66: (64, 65)}.items():    # relatives across the tiles
        G[child] = np.where(rng.random(600) < 0.5, G[p1], G[p2])
    G[100] = G[7]
    b = handle(ba, G)
    thr = 2 ** -4.5
    got = ba.bed_king(b, thr_king=thr)
    want = ref.table(G, thr=thr)
    kc.assert_same_table(got, want)
    assert 4 <= got["KINSHIP"].size < 150 * 149 // 2 and (got["KINSHIP"] >= thr).all()
    again = ba.bed_king(b, thr_king=thr)
    for name in got:
        assert got[name].tobytes() == again[name].tobytes(), name
    everything, twice = ba.bed_king(b), ba.bed_king(b)
    for name in everything:
        assert everything[name].tobytes() == twice[name].tobytes(), name
    np.testing.assert_array_equal(np.lexsort((everything["I2"], everything["I1"])), np.arange(everything["I1"].size))


def test_second_batch_and_growing_table(ba):
    """65 sample tiles are 2 145 tile pairs: more than the 2 048 whose statistics are held at once, so the last tile rows
    come in a second batch behind the rows of the first; the filtered table is allocated for the rows of the first batch
    and moved to a larger allocation when the second adds its own"""
    G = kc.random_codes(4100, 70, 0.03, seed=31)
    G[4098] = G[4097]                                   # a row among the four samples of the last tile
    b = handle(ba, G)
    thr = 0.12
    got = ba.bed_king(b, thr_king=thr)
    want = ref.table(G, thr=thr)
    assert 4 * 65536 < want["KINSHIP"].size < 4100 * 4099 // 4
    assert (want["I1"] >= 51 * 64).sum() > 1000 and (want["I1"] >= 4096).any()     # tile rows 51 .. 64 are the second batch
    kc.assert_same_table(got, want)


@pytest.fixture()
def related_bed(tmp_path):
    """example.bed with sample 0 made a relative of samples 1 and 2, as the reference's test prepares it"""
    G = kc.related_example()
    path = str(tmp_path / "rel.bed")
    with open(path, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(kc.encode_payload(G).tobytes())
    for ext in (".bim", ".fam"):
        shutil.copy(os.path.join(kc.GOLDEN, "example" + ext), path[:-4] + ext)
    return path, G


def test_reference_expectations(ba, related_bed):
    """tests/testthat/test-3-plink-QC.R:90-114 of the reference through bed_kingQC"""
    path, G = related_bed
    obj = ba.bed(path)
    t = ba.bed_kingQC(obj, thr_king=0.177, make_bed=False)
    assert t["KINSHIP"].size == 1 and t["KINSHIP"][0] > 0.177
    assert t["KINSHIP"][0] == 0.18879387938793880 and t["HETHET"][0] == 720 and t["IBS0"][0] == 0
    assert (t["I1"][0], t["I2"][0]) == (0, 2)
    assert (t["FID1"][0], t["IID1"][0], t["FID2"][0], t["IID2"][0]) == ("POP1", "IND0", "POP1", "IND2")
    assert ba.bed_kingQC(obj, thr_king=0.3, make_bed=False)["KINSHIP"].size == 0
    full = ba.bed_king(obj)
    order = np.argsort(-full["KINSHIP"], kind="stable")
    assert [(int(full["I1"][k]), int(full["I2"][k])) for k in order[:3]] == [(0, 2), (0, 1), (168, 191)]
    assert full["KINSHIP"][order[1]] == 0.17349234923492352
    keep, removed = ba.king_norel(t, obj.nrow)
    assert removed.tolist() == [2]
    out = ba.bed_kingQC(obj, thr_king=0.177)
    assert out == path[:-4] + "_norel.bed"
    back = ba.bed(out)
    assert (back.nrow, back.ncol) == (516, 4542)
    ids = list(zip(back.fam["family_ID"], back.fam["sample_ID"]))
    assert ("POP1", "IND2") not in ids and ("POP1", "IND0") in ids and ("POP1", "IND1") in ids
    np.testing.assert_array_equal(ba.bed_to_bytes(back), G[keep].astype(np.uint8))
    with pytest.raises(FileExistsError, match="already exists"):
        ba.bed_kingQC(obj, thr_king=0.177)
    other = ba.bed_kingQC(obj, thr_king=0.177, bedfile_out=path[:-4] + "_other.bed")
    assert ba.bed(other).nrow == 516


def test_example_missing(ba):
    obj = ba.bed(os.path.join(kc.GOLDEN, "example-missing.bed"))
    t = ba.bed_king(obj)
    assert t["KINSHIP"].size == 19900 and (~np.isfinite(t["KINSHIP"])).sum() == 397
    kc.assert_same_table({k: v for k, v in t.items() if k[1:3] != "ID"}, ref.table(kc.read_golden("example-missing")[0]))
    assert ba.bed_kingQC(obj, thr_king=2 ** -4.5, make_bed=False)["KINSHIP"].size == 5689
    assert ba.bed_kingQC(obj, make_bed=False)["KINSHIP"].size == 4540


def test_refusals(ba, monkeypatch, tmp_path):
    G = kc.random_codes(20, 40, 0.03, seed=21)
    b = handle(ba, G)
    with pytest.raises(ba.BsnError, match="at least 2 samples"):
        ba.bed_king(b, ind_row=np.array([3]))
    with pytest.raises(ba.BsnError, match="at least 1 variant"):
        ba.bed_king(b, ind_col=np.zeros(0, dtype=np.int64))
    monkeypatch.setenv("BSN_NO_SMAJ", "1")
    with pytest.raises(ba.BsnError, match="no room for the sample-major operand"):
        ba.bed_king(handle(ba, G))
    monkeypatch.delenv("BSN_NO_SMAJ")
    dosage = ba.FBM_code256(np.full((8, 5), 50, dtype=np.uint8), ba.CODE_DOSAGE)
    assert dosage.bits == 8
    with pytest.raises(ba.BsnError, match="bed_king is not available for this handle: it needs a 2-bit genotype image"):
        ba.bed_king(dosage)
    shutil.copy(os.path.join(kc.GOLDEN, "example-missing.bed"), tmp_path / "ooc.bed")
    for ext in (".bim", ".fam"):
        shutil.copy(os.path.join(kc.GOLDEN, "example-missing" + ext), tmp_path / ("ooc" + ext))
    pitch = (200 + 3) // 4 + 255 & ~255
    monkeypatch.setenv("BSN_IMAGE_BUDGET", str(130 * pitch))
    ooc = ba.bed(str(tmp_path / "ooc.bed"))
    monkeypatch.delenv("BSN_IMAGE_BUDGET")
    assert ooc.streamed
    with pytest.raises(ba.BsnError, match="bed_king needs the genotype image resident on the device"):
        ba.bed_king(ooc)
    with pytest.raises(ValueError, match="attached to a file"):
        ba.bed_kingQC(b)
