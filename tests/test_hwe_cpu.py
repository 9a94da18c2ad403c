"""The exact Hardy-Weinberg test and the host logic of bed_plinkQC / bed_plinkRmSamples without a GPU.

The CPU statement (tests/native/hwe_ref.cpp over bigsnpr_amd/csrc/hwe_step.hpp, the header the kernel is compiled from) is
compared with an exact reference: P(het = h) is proportional to 2^h / (homr! h! homc!), here the integers
2^h N! / (homr! h! homc!) (the two ends of the range from factorials, the ones in between by exact integer division, the
chain checked against the far end), summed as integers and divided once as a Fraction.  The tie rule of the statement (a
term within 1e-8 of the observed one counts as equal) is applied in exact arithmetic, and the reference asserts that no
case has two terms whose ratio lies in (1, 1 + 1e-6), so the rule never decides a case.

Tolerances.  N <= 40: at most 20 steps from the observed term, three roundings a step, two sums and a division stay below
2e-14 relative; 1e-12 leaves margin.  N <= 5 000: at most 2 500 steps x 3 roundings x 2^-53 < 1e-12 on every term, and the
same again for the sums; 1e-11.  The N = 20 000 case of the DBL_MIN stop: the steps the statement itself reports x 3 x
2^-53, doubled for the sums."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

import hwe_ref as ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TIE = Fraction(1, 10 ** 8)
GAP = Fraction(1, 10 ** 6)


def exact_p(hom1, het, hom2, midp=False):
    """the p-value as a Fraction (None for N = 0), by integer factorials"""
    N = hom1 + het + hom2
    if N == 0:
        return None
    lo = min(hom1, hom2)
    rare = 2 * lo + het
    if rare == 0:
        return Fraction(1)        # (the statement's rule for a monomorphic variant, mid-p included)
    fN = math.factorial(N)

    def weight(h):
        homr = (rare - h) // 2
        return (fN << h) // (math.factorial(homr) * math.factorial(h) * math.factorial(N - h - homr))

    # The integer weights of h = rare mod 2, ..., rare.  Only the two ends are formed from factorials: in between, the
    # quotient of neighbouring weights is the integer identity w(h + 2) (h + 2) (h + 1) = w(h) 4 homr homc, every
    # division below is checked to be exact, and the chain has to arrive at the factorial form of w(rare).
    hs = list(range(rare % 2, rare + 1, 2))
    ws = [weight(hs[0])]
    for h in hs[:-1]:
        homr = (rare - h) // 2
        w, rem = divmod(ws[-1] * (4 * homr * (N - h - homr)), (h + 2) * (h + 1))
        assert rem == 0
        ws.append(w)
    assert ws[-1] == weight(rare)
    w_obs = ws[hs.index(het)]
    total, tail2 = 0, 0           # tail2: twice the tail, so that the halves of mid-p stay integers
    for h, w in zip(hs, ws):
        total += w
        if h == het:
            tail2 += w if midp else 2 * w
            continue
        # (ratios against the observed weight, as integer comparisons: r = w / w_obs)
        assert w == w_obs or abs(w - w_obs) * GAP.denominator > w_obs, \
            "two terms of (%d, %d, %d) lie within 1e-6 of each other" % (hom1, het, hom2)
        if midp and abs(w - w_obs) * TIE.denominator <= w_obs:
            tail2 += w
        elif w * TIE.denominator <= w_obs * (TIE.denominator + 1):
            tail2 += 2 * w
    return Fraction(tail2, 2 * total)


def all_triples(nmax):
    return [(a, b, N - a - b) for N in range(nmax + 1) for a in range(N + 1) for b in range(N - a + 1)]


@pytest.fixture(scope="module")
def small():
    t = all_triples(40)
    assert len(t) == 12341
    return np.array(t, dtype=np.int32).T


@pytest.mark.parametrize("midp", [False, True])
def test_every_table_up_to_40_genotypes(small, midp):
    got = ref.exact(small, midp)
    worst = 0.0
    for j in range(small.shape[1]):
        want = exact_p(*[int(v) for v in small[:, j]], midp=midp)
        if want is None:
            assert np.isnan(got[j])
            continue
        err = abs(Fraction(float(got[j])) - want) / want
        worst = max(worst, float(err))
        assert err <= Fraction(1, 10 ** 12), (small[:, j], got[j], float(want))
    print("midp %d: largest relative error %.3g" % (midp, worst))


# a dozen tables up to N = 5 000: common and rare alleles, excess and lack of heterozygotes, both parities of `rare`, the
# observed count at either end of its range
LARGE = [(1200, 2400, 1400), (1250, 2500, 1250), (10, 400, 4590), (0, 100, 4900), (3, 93, 4904), (900, 1700, 2400),
         (1300, 2200, 1500), (50, 2001, 2949), (1, 1, 4998), (0, 1, 4999), (700, 2601, 1699), (1666, 1667, 1667)]


@pytest.mark.parametrize("midp", [False, True])
def test_large_tables(midp):
    assert len(LARGE) >= 12 and all(sum(t) <= 5000 for t in LARGE)
    got = ref.exact(np.array(LARGE).T, midp)
    for t, g in zip(LARGE, got):
        want = exact_p(*t, midp=midp)
        assert abs(Fraction(float(g)) - want) / want <= Fraction(1, 10 ** 11), (t, g, float(want))


def test_the_two_alleles_are_interchangeable():
    t = np.array(LARGE).T
    np.testing.assert_array_equal(ref.exact(t), ref.exact(t[::-1]))
    np.testing.assert_array_equal(ref.exact(t, True), ref.exact(t[::-1], True))


def test_edge_cases():
    assert np.isnan(ref.exact1(0, 0, 0)) and np.isnan(ref.exact1(0, 0, 0, True))
    for t in ((7, 0, 0), (0, 0, 7), (INT32_MAX, 0, 0)):                       # monomorphic
        assert ref.exact1(*t) == 1.0 and ref.exact1(*t, True) == 1.0
    # het = 0 with both alleles present; rare = 1 (one table only: p = 1, mid-p 0.5); both parities of rare
    assert ref.exact1(1, 0, 9) == float(exact_p(1, 0, 9))
    assert ref.exact1(0, 1, 9) == 1.0 and ref.exact1(0, 1, 9, True) == 0.5
    for t in ((3, 4, 13), (3, 5, 12), (0, 6, 14), (0, 7, 13)):
        for midp in (False, True):
            assert ref.exact1(*t, midp) == pytest.approx(float(exact_p(*t, midp)), rel=1e-13)
    # a p-value never exceeds 1 (the observed table is the most likely one and every other one ties below 1 + 1e-8)
    assert ref.exact1(1, 2, 1) == 1.0


INT32_MAX = 2 ** 31 - 1


def test_overflow_gives_zero():
    """a term that reaches inf: the true p-value is below about 1e-300 and the statement returns 0"""
    for t in ((100000, 0, 100000), (0, 200000, 0), (2400, 199, 2401)):
        assert ref.exact1(*t) == 0.0 and ref.exact1(*t, True) == 0.0
        total_down, _, total_up, _ = ref.walks(*t)
        assert np.isinf(total_down) or np.isinf(total_up)
    want = exact_p(2400, 199, 2401)
    assert 0 < want < Fraction(1, 10 ** 300)


def test_walks_stop_below_dbl_min():
    """N = 20 000 with het at its expectation: both walks end when their term falls below DBL_MIN, long before h leaves
    its range, and what they leave out does not show in the result"""
    t = (5000, 10000, 5000)
    p, steps = ref.exact(np.array(t).reshape(3, 1), steps=True)
    full_range = (2 * t[0] + t[1]) // 2
    assert 1000 < steps[0] < full_range // 2, steps
    want = exact_p(*t)
    tol = 2 * 3 * int(steps[0]) * 2.0 ** -53
    assert abs(Fraction(float(p[0])) - want) / want <= Fraction(tol), (p, float(want))
    # the terms beyond the stop, exactly: below DBL_MIN each, relative to the observed one
    total_down, tail_down, total_up, tail_up = ref.walks(*t)
    assert np.isfinite([total_down, tail_down, total_up, tail_up]).all()


def test_filter_expressions():
    assert ref.too_many_missing(11, 100, 0.1) and not ref.too_many_missing(10, 100, 0.1)
    assert not ref.too_many_missing(100, 100, 1.0) and ref.too_many_missing(1, 100, 0.0)
    assert ref.missing_rate(1, 3) == 1 / 3
    assert ref.maf(10, 20, 70) == 40 / 200 and ref.maf(70, 20, 10) == 40 / 200
    assert np.isnan(ref.maf(0, 0, 0))
    assert ref.maf_too_low(float("nan"), 0.01) and not ref.maf_too_low(float("nan"), 0.0)
    assert ref.maf_too_low(0.0099, 0.01) and not ref.maf_too_low(0.01, 0.01)
    assert ref.rejected(1e-51, 1e-50) and not ref.rejected(1e-50, 1e-50)
    assert not ref.rejected(0.0, 0.0) and not ref.rejected(float("nan"), 1e-50)


# ---- the host logic of bed_plinkQC / bed_plinkRmSamples on the golden files, the device calls replaced ---------------------
def file_object(prefix):
    """a `bed` object of the golden files without a device handle"""
    from bigsnpr_amd.bed import _count_lines, bed
    b = bed.__new__(bed)
    b._h = b._map = b._fam = None
    b.bedfile = os.path.join(GOLDEN, prefix + ".bed")
    b.nrow, b.ncol = _count_lines(b.famfile), _count_lines(b.bimfile)
    return b


def test_classes_of_the_golden_fam():
    from bigsnpr_amd.qc import qc_classes
    fam = file_object("example").fam
    aff = np.asarray(fam["affection"])
    assert set(aff) == {1, 2}
    cls = qc_classes(fam)
    np.testing.assert_array_equal(cls, np.where(aff == 1, 0, 1))             # all founders; the controls are tested
    np.testing.assert_array_equal(qc_classes(fam, hwe_controls_only=False), 0)
    # children; and phenotypes that are not case / control
    fam2 = {k: np.array(v, copy=True) for k, v in fam.items()}
    fam2["paternal_ID"][[3, 5]] = "IND0"
    fam2["maternal_ID"][[4, 5]] = "IND1"
    cls2 = qc_classes(fam2)
    np.testing.assert_array_equal(cls2[[3, 4, 5]], 2)
    np.testing.assert_array_equal(np.delete(cls2, [3, 4, 5]), np.delete(cls, [3, 4, 5]))
    np.testing.assert_array_equal(qc_classes(fam2, founders_only=False), cls)
    fam3 = dict(fam, affection=np.where(aff == 1, 0.37, 1.5))
    np.testing.assert_array_equal(qc_classes(fam3), 0)
    np.testing.assert_array_equal(qc_classes(file_object("example-missing").fam), 0)     # all -9: no control, all tested
    fam4 = dict(fam, affection=np.array(["NA"] * aff.size))
    np.testing.assert_array_equal(qc_classes(fam4), 0)


def test_autosomes():
    from bigsnpr_amd.qc import autosomes
    chrs = ["1", "22", "23", "0", "X", "chr7", "CHR22", "chrX", "chr", "MT", "1_random", "-1", "chr0"]
    np.testing.assert_array_equal(autosomes(chrs), [1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0])
    assert autosomes(file_object("example").map["chromosome"]).all()
    assert autosomes(np.array([1, 5, 26])).tolist() == [True, True, False]


def test_plinkQC_host_logic(monkeypatch, tmp_path):
    from bigsnpr_amd import qc
    b = file_object("example")
    calls = []

    def fake_call(im, ir, ic, cls, maf, geno, mind, hwe, midp):
        calls.append(dict(ir=ir, ic=ic, cls=np.array(cls), args=(maf, geno, mind, hwe, midp)))
        keep_row, keep_col = np.ones(ir.size, dtype=bool), np.ones(ic.size, dtype=bool)
        keep_row[[1, 7]] = False
        keep_col[[0, 2, 5]] = False
        stats = np.zeros((ic.size, 3))
        stats[:, 0] = 0.0          # missing rate
        stats[:, 1] = 0.3          # maf
        stats[:, 2] = 0.5          # p
        stats[0] = (0.5, 0.3, 0.5)
        stats[2] = (0.0, 0.001, 0.5)
        stats[5] = (0.0, np.nan, 1e-60)
        return keep_row, keep_col, np.linspace(0, 0.2, ir.size), stats

    written = []
    monkeypatch.setattr(qc, "_qc_call", fake_call)
    monkeypatch.setattr(qc, "_write_subset", lambda im, out, ir, ic: written.append((out, ir, ic)) or out)
    rep = qc.bed_plinkQC(b, make_bed=False, ind_col=np.arange(10, 60))
    c = calls[-1]
    assert c["args"] == (0.01, 0.1, 0.1, 1e-50, False)                       # the reference's defaults
    np.testing.assert_array_equal(c["cls"], qc.qc_classes(b.fam))
    np.testing.assert_array_equal(rep["ind_row"], np.delete(np.arange(b.nrow), [1, 7]))
    np.testing.assert_array_equal(rep["ind_col"], np.delete(np.arange(10, 60), [0, 2, 5]))
    assert rep["removed"] == dict(autosome=0, mind=2, geno=1, hwe=1, maf=2)
    # rows selected: the classes follow the selection
    qc.bed_plinkQC(b, make_bed=False, ind_row=np.arange(100, 300), hwe_controls_only=False, maf=0, hwe=0)
    assert calls[-1]["cls"].shape == (200,) and calls[-1]["args"][0] == 0 and calls[-1]["args"][3] == 0
    # the default output path, written through the one writer; an existing file is refused before anything is computed
    out = qc.bed_plinkQC(b, bedfile_out=str(tmp_path / "x.bed"))
    assert out == str(tmp_path / "x.bed") and written[-1][0] == out
    np.testing.assert_array_equal(written[-1][1], np.delete(np.arange(b.nrow), [1, 7]))
    np.testing.assert_array_equal(written[-1][2], np.delete(np.arange(b.ncol), [0, 2, 5]))
    (tmp_path / "x.fam").write_text("")
    n_calls = len(calls)
    with pytest.raises(FileExistsError, match="x.fam"):
        qc.bed_plinkQC(b, bedfile_out=str(tmp_path / "x.bed"))
    assert len(calls) == n_calls
    # autosome_only is applied before the device sees anything
    b._map = dict(b.map, chromosome=np.where(np.arange(b.ncol) % 3 == 0, "X", "chr2"))
    rep = qc.bed_plinkQC(b, make_bed=False, autosome_only=True, ind_col=np.arange(30))
    np.testing.assert_array_equal(calls[-1]["ic"], [j for j in range(30) if j % 3])
    assert rep["removed"]["autosome"] == 10
    b._map = None


def test_default_output_name(monkeypatch):
    from bigsnpr_amd import qc
    b = file_object("example")
    seen = []
    monkeypatch.setattr(qc, "_check_out", lambda path: seen.append(path) or (_ for _ in ()).throw(FileExistsError(path)))
    with pytest.raises(FileExistsError):
        qc.bed_plinkQC(b)
    assert seen == [os.path.join(GOLDEN, "example_QC.bed")]


def test_plinkRmSamples_host_logic(monkeypatch, tmp_path):
    from bigsnpr_amd import qc
    b = file_object("example")
    fam = b.fam
    written = []
    monkeypatch.setattr(qc, "_write_subset", lambda im, out, ir, ic: written.append((out, ir, ic)) or out)
    out = str(tmp_path / "rm.bed")
    gone = [0, 5, 516]
    table = dict(fid=fam["family_ID"][gone], iid=fam["sample_ID"][gone])
    assert qc.bed_plinkRmSamples(b, out, table) == out
    np.testing.assert_array_equal(written[-1][1], np.delete(np.arange(b.nrow), gone))
    np.testing.assert_array_equal(written[-1][2], np.arange(b.ncol))
    # rows with other columns around, columns named by position; files, several of them, with a header
    rows = [["x", fam["sample_ID"][k], fam["family_ID"][k]] for k in gone]
    qc.bed_plinkRmSamples(b, out, rows, col_family_ID=2, col_sample_ID=1)
    np.testing.assert_array_equal(written[-1][1], np.delete(np.arange(b.nrow), gone))
    f1, f2 = tmp_path / "a.txt", tmp_path / "b.txt"
    f1.write_text("FID IID\n%s %s\n" % (fam["family_ID"][3], fam["sample_ID"][3]))
    f2.write_text("FID IID\n%s\t%s\n\n" % (fam["family_ID"][9], fam["sample_ID"][9]))
    qc.bed_plinkRmSamples(b, out, [str(f1), str(f2)], header=True)
    np.testing.assert_array_equal(written[-1][1], np.delete(np.arange(b.nrow), [3, 9]))
    with pytest.raises(ValueError, match="family.ID 'POP1', sample.ID 'NOBODY'"):
        qc.bed_plinkRmSamples(b, out, [["POP1", "NOBODY"]])
    with pytest.raises(ValueError, match="must be a table"):
        qc.bed_plinkRmSamples(b, out, 3)
    (tmp_path / "rm.bim").write_text("")
    with pytest.raises(FileExistsError, match="rm.bim"):
        qc.bed_plinkRmSamples(b, out, table)
