"""The host side of snp_readBGEN / snp_prodBGEN without a GPU: format_snp_id and snp_readBGI on the reference's example
index and on a written file, the header and argument error strings, and the CPU twin of bgen_step.hpp (table rule, info /
freq including nona == 0, the random rule) against a NumPy restatement, bit for bit; and the conditions under which the
files of tests/test_gpu_bgen_shapes.py (tests/helpers/bgen_cases.py) reach what they are there for."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bgen_cases as bc  # noqa: E402
import bgen_inputs as bi  # noqa: E402
import bgen_ref as ref  # noqa: E402
from test_impute_cpu import philox4x32_10, unit_open  # noqa: E402

TAG = 0x4247454E
K_TABLE = 511   # kTable of bgen_step.hpp: 2 p0 + p1 = 0 .. 510 (test_table_rule holds the table itself to it)


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    return bi.example_files(tmp_path_factory.mktemp("bgen"))


def test_format_snp_id(ba):
    assert ba.format_snp_id(["1_88169_C_T", "01_88169_C_T", "X1_5_A_G"]) == ["01_88169_C_T", "01_88169_C_T", "X1_5_A_G"]
    with pytest.raises(ValueError, match="Wrong format of some variants."):
        ba.format_snp_id(["1_88169_C_T", "001_88169_C_T"])


def test_readBGI_on_the_fixture(ba, example):
    tab = ba.snp_readBGI(example + ".bgi")
    assert len(tab["rsid"]) == 199 and set(tab) == {"chromosome", "position", "rsid", "number_of_alleles", "allele1",
                                                    "allele2", "file_start_position", "size_in_bytes"}
    assert tab["file_start_position"].dtype == np.int64 and (tab["number_of_alleles"] == 2).all()
    ids = ["%s_%d_%s_%s" % (c, p, a, b) for c, p, a, b in zip(tab["chromosome"], tab["position"], tab["allele1"], tab["allele2"])]
    pick = [5, 150, 3, 77]
    sub = ba.snp_readBGI(example + ".bgi", [ids[k].lstrip("0") for k in pick])   # "01_..." and "1_..." both match
    assert list(sub["file_start_position"]) == [tab["file_start_position"][k] for k in pick]
    assert sub["rsid"] == [tab["rsid"][k] for k in pick]
    with pytest.raises(ValueError, match="Some variants have not been found"):
        ba.snp_readBGI(example + ".bgi", [ids[0], "01_123_A_C"])
    assert ba.check_bgen_format(example) == 500


def test_readBGI_on_a_written_file(ba, tmp_path):
    p0, p1, miss = bi.probabilities(21, 6, seed=4)
    path = str(tmp_path / "w.bgen")
    var = bi.write_bgen(path, p0, p1, miss)
    tab = ba.snp_readBGI(path + ".bgi", [v["snp_id"] for v in reversed(var)])
    assert list(tab["file_start_position"]) == [v["offset"] for v in reversed(var)]
    assert ba.check_bgen_format(path) == 21
    cols, dos, ids, sums = bi.decode_file(path, [v["offset"] for v in var])
    assert ids == [v["id"] for v in var] and cols.shape == (21, 6)
    assert np.array_equal(cols == 3, miss)


def test_header_errors(ba, tmp_path):
    p0, p1, miss = bi.probabilities(5, 2, seed=1)
    for kw, msg in ((dict(magic=b"nope"), "is not a BGEN file."), (dict(flags=2 | (2 << 2)), "is not compressed with zlib."),
                    (dict(flags=1 | (1 << 2)), "is not using Layout 2.")):
        path = str(tmp_path / "bad.bgen")
        bi.write_bgen(path, p0, p1, miss, **kw)
        with pytest.raises(ValueError, match="'%s' %s" % (path.replace(".", r"\."), msg.replace(".", r"\."))):
            ba.check_bgen_format(path)


def test_argument_errors_need_no_gpu(ba, tmp_path):
    p0, p1, miss = bi.probabilities(5, 2, seed=1)
    path = str(tmp_path / "ok.bgen")
    var = bi.write_bgen(path, p0, p1, miss)
    ids = [v["snp_id"] for v in var]
    for f in (ba.snp_readBGEN, lambda *a, **k: ba.snp_prodBGEN(a[0], np.ones(2), *a[1:], **k)):
        with pytest.raises(TypeError, match="'list_snp_id' is not of class 'list'."):
            f(path, tuple(ids))
        with pytest.raises(ValueError, match="Wrong format of some variants."):
            f(path, [["001_5_A_C", ids[1]]])
        with pytest.raises(ValueError, match="ind_row >= 1 & ind_row <= N"):
            f(path, [ids], ind_row=[0, 5])
        with pytest.raises(ValueError, match="ind_row >= 1 & ind_row <= N"):
            f(path, [ids], ind_row=[-1])
        with pytest.raises(ValueError, match="must be '.bgen'"):
            f(path + ".bgi", [ids])
        with pytest.raises(ValueError, match="Some variants have not been found"):
            f(path, [[ids[0], "01_999999_A_C"]])
        with pytest.raises(ValueError, match="same length"):
            f([path, path], [ids])
    with pytest.raises(ValueError, match="nrow.beta. == sum.sizes."):
        ba.snp_prodBGEN(path, np.ones(3), [ids])


# ---- the twin of bgen_step.hpp against numpy ------------------------------------------------------------------------------
def test_table_rule():
    lib = ref.load("bgen_ref")
    tab = np.array([lib.bgen_table_byte(k) for k in range(511)])
    assert np.array_equal(tab, 207 - np.round(np.arange(511) * 100 / 255).astype(np.int64))
    assert np.array_equal(tab, bi.DECODE_BYTES) and tab[0] == 207 and tab[510] == 7
    frac = np.arange(511) * 100 / 255 % 1
    assert np.abs(frac - 0.5).min() > 0.009      # no tie: rounding half up, half even and floor(x + 0.5) agree
    import bigsnpr_amd.bgen as host
    assert np.array_equal(host.DECODE_BYTES, tab) and np.array_equal(host.DECODE_DOSAGE, np.arange(510, -1, -1) / 255)
    # the grid index of every FBM byte is what CODE_DOSAGE decodes it to, in hundredths about 1
    import bigsnpr_amd as ba
    for b in range(256):
        g = lib.bgen_grid_of_byte(b)
        v = ba.CODE_DOSAGE[b]
        assert (g == -128) if np.isnan(v) else (g == int(round(100 * v)) - 100), b


def test_info_freq_bit_for_bit():
    rng = np.random.default_rng(3)
    sums = []
    for _ in range(200):
        n = int(rng.integers(1, 5000))
        p0, p1, miss = bi.probabilities(n, 1, seed=int(rng.integers(1 << 30)), confident=float(rng.random()))
        k = 2 * p0[:, 0].astype(np.int64) + p1[:, 0]
        ok = ~miss[:, 0]
        sums.append((ok.sum(), k[ok].sum(), (255 * (4 * p0[:, 0].astype(np.int64) + p1[:, 0]) - k * k)[ok].sum()))
    sums += [(0, 0, 0), (7, 0, 0), (7, 7 * 510, 0)]
    sums = np.array(sums, dtype=np.int64)
    info, freq = bi.info_freq(sums)
    for s, a, b in zip(sums, info, freq):
        got = ref.info_freq(*s)
        assert np.array_equal(np.array(got), np.array([a, b]), equal_nan=True), (s, got, a, b)
    assert np.isnan(ref.info_freq(0, 0, 0)).all()           # nona == 0: NaN twice, as the reference's arithmetic gives
    assert ref.info_freq(7, 0, 0)[1] == 1.0 and np.isnan(ref.info_freq(7, 0, 0)[0])


def test_random_rule_bit_for_bit():
    lib = ref.load("bgen_ref")
    seed = 20240611
    i = np.arange(300, dtype=np.uint64)
    j = np.full(300, 17, dtype=np.uint64)
    o = philox4x32_10([i, j, np.full(300, TAG, dtype=np.uint64), np.zeros(300, dtype=np.uint64)],
                      (seed & 0xFFFFFFFF, seed >> 32))
    u = unit_open(o[0], o[1])
    assert all(lib.bgen_unit(seed, int(a), 17) == float(b) for a, b in zip(i, u))
    assert lib.bgen_unit(seed + 1, 0, 17) != lib.bgen_unit(seed, 0, 17)
    p0, p1, _ = bi.probabilities(300, 1, seed=2)
    p0, p1 = p0[:, 0].astype(np.int64), p1[:, 0].astype(np.int64)
    first = u * 255 - p0
    want = np.where(first < 0, 0, np.where(first < p1, 1, 2))
    got = [lib.bgen_random_call(float(a), int(b), int(c)) for a, b, c in zip(u, p0, p1)]
    assert list(want) == got
    # a probability of 255 is that genotype, whatever u
    for uu in (1e-300, 0.5, 1 - 2.0 ** -53):
        assert lib.bgen_random_call(uu, 255, 0) == 0 and lib.bgen_random_call(uu, 0, 255) == 1 and lib.bgen_random_call(uu, 0, 0) == 2


def test_variant_twin_against_numpy(tmp_path):
    p0, p1, miss = bi.probabilities(85, 3, seed=9, missing=0.1)
    path = str(tmp_path / "v.bgen")
    var = bi.write_bgen(path, p0, p1, miss)
    rows = np.array([84, 0, 0, 17, 3], dtype=np.int64)
    cols, _, _, sums = bi.decode_file(path, [v["offset"] for v in var], rows)
    for j in range(3):
        block = np.frombuffer(bi.inflated_block(p0[:, j], p1[:, j], miss[:, j]), dtype=np.uint8)
        got, s = ref.variant(block, 85, rows, bi.DECODE_BYTES, 1, 0, j)
        assert np.array_equal(got, cols[:, j]) and np.array_equal(s, sums[j])


# ---- the conditions of tests/test_gpu_bgen_shapes.py, proved without a GPU -----------------------------------------------------
def random_bytes(f, rows, seed, col0=0):
    """what read_as = "random" makes of a written file at global columns col0 .., by the twin of bgen_step.hpp"""
    out = np.empty((len(rows), f["K"]), dtype=np.uint8)
    for j, block in enumerate(bc.blocks(f)):
        out[:, j], _ = ref.variant(block, f["N"], rows, bi.DECODE_BYTES, 0, seed, col0 + j)
    return out


def test_product_cases_take_a_second_turn(tmp_path):
    """A, B, C: more than kProdRows = 128 variants in a block, so the v0 loop of k_bgen_prod goes round again"""
    f = bc.case_ab(tmp_path)
    assert (f["N"], f["K"]) == (257, 300)
    for bs in f["block_sizes_A"] + f["block_sizes_B"][:2]:
        assert min(bs, f["K"]) > bc.PROD_ROWS
    assert [min(129, f["K"] - k0) for k0 in range(0, f["K"], 129)] == [129, 129, 42]      # a turn of one row, three blocks
    assert [min(128, 300 - v0) for v0 in range(0, 300, 128)] == [128, 128, 44]
    assert f["block_sizes_B"][2] == 7 and f["K"] % 7 != 0                                 # k0 = 7, 14 ...: the last block short
    # ncol at one tile, one past it, and two whole tiles
    assert [n % bc.PROD_COLS for n in f["ncols_A"]] == [0, 1, 0] and f["ncols_A"][2] == 2 * bc.PROD_COLS
    _, X, _, _ = bi.decode_file(f["path"], f["offs"])
    assert 0 < np.isnan(X).any(axis=1).sum() < f["N"]
    c = bc.case_c(tmp_path)
    sizes = [g["K"] for g in c["files"]]
    assert sizes == [5, 1, 130] and min(c["block_size"], sizes[2]) > bc.PROD_ROWS and sum(sizes[:2]) == 6
    assert c["beta"].shape == (sum(sizes), 9) and np.array_equal(c["beta"], np.rint(c["beta"])) and np.abs(c["beta"]).max() == 3
    assert f["beta_B"].shape == (300, 9) and np.array_equal(f["beta_B"], np.rint(f["beta_B"])) and np.abs(f["beta_B"]).max() == 3


def test_repeat_case_draws_by_position(tmp_path):
    """B: some file sample is listed twice, is uncertain (0 < p0 < 255) in some variant, and its two positions draw
    different calls there: the draw is keyed by the position in ind_row, not by the sample"""
    f = bc.case_ab(tmp_path)
    rows = f["rows_B"]
    assert rows.size == 300 and np.unique(rows).size < 300
    got = random_bytes(f, rows, f["seed"])
    found = 0
    for s in np.unique(rows):
        at = np.flatnonzero(rows == s)
        if at.size < 2:
            continue
        unsure = (f["p0"][s] > 0) & (f["p0"][s] < 255) & ~f["miss"][s]
        found += int((unsure & (got[at[0]] != got[at[1]])).any())
    assert found > 0
    assert not np.array_equal(got, random_bytes(f, rows, f["seed"] + 1))
    # the third file of C starts at global column 6: its draws are not those of column 0
    c = bc.case_c(tmp_path)
    g = c["files"][2]
    assert not np.array_equal(random_bytes(g, c["rows"], c["seed"], 6), random_bytes(g, c["rows"], c["seed"], 0))


def test_stride_case_is_past_the_grid(tmp_path):
    """D: more positions than the 1 024 x 256 threads k_bgen_grid8 is launched with"""
    f = bc.case_d(tmp_path)
    assert f["rows"].size == bc.GRID8_THREADS + 300 > 1024 * 256 and f["K"] == 3
    assert (f["rows"].size + 255) // 256 > 1024
    assert f["miss"][f["rows"]].any() and f["rows"].min() >= 0 and f["rows"].max() < f["N"]


def test_refusal_cases_have_one_sample_past_the_table(tmp_path):
    """E: exactly one (sample, variant) has 2 p0 + p1 == 511, the control's largest value is 510, the table's last"""
    e = bc.case_e(tmp_path)
    k_bad = 2 * e["bad"]["p0"].astype(np.int64) + e["bad"]["p1"]
    k_good = 2 * e["good"]["p0"].astype(np.int64) + e["good"]["p1"]
    live = ~e["bad"]["miss"]
    assert np.argwhere((k_bad >= K_TABLE) & live).tolist() == [[e["sample"], e["variant"]]]
    assert k_bad[e["sample"], e["variant"]] == 511 == K_TABLE
    assert k_good[live].max() == 510 == k_good[e["sample"], e["variant"]] and bi.DECODE_BYTES.size == 511
    assert e["sample"] not in e["without"] and np.unique(e["without"]).size < e["without"].size
    assert e["variant"] // e["block"] == 2 and e["bad"]["K"] == 7 and e["bad"]["N"] == 21   # the third of four blocks
    cols, _, _, _ = bi.decode_file(e["good"]["path"], e["good"]["offs"])
    assert cols[e["sample"], e["variant"]] == 7                                             # dosage 0.00
    e3 = bc.case_e_files(tmp_path)
    assert len(e3["bad"]) == 3 and e3["bad"][:2] == e3["good"][:2]
    k = 2 * e3["bad"][2]["p0"].astype(np.int64) + e3["bad"][2]["p1"]
    assert ((k == 511) & ~e3["bad"][2]["miss"]).sum() == 1
    assert all((2 * g["p0"].astype(np.int64) + g["p1"]).max() <= 510 for g in e3["good"])


def test_column_limit_and_cut_file(tmp_path):
    """F: 65 535 tiles of 8 columns; G: the offsets and the cut that the host walk must refuse"""
    f = bc.case_f(tmp_path)
    assert f["ncol"] == 65535 * 8 == 524280 and (f["N"], f["K"]) == (1, 1) and not f["miss"].any()
    g = bc.case_g(tmp_path)
    last = g["var"][-1]
    assert last["offset"] < g["cut_size"] < last["offset"] + last["size"] == g["size"] and os.path.getsize(g["cut"]) == g["cut_size"]
    assert g["moved"]["at"][1] == g["size"] and g["moved"]["beyond"][1] > g["size"]
    import sqlite3
    for path, off in g["moved"].values():
        assert os.path.getsize(path) == g["size"]
        db = sqlite3.connect(path + ".bgi")
        assert max(r[0] for r in db.execute("SELECT file_start_position FROM Variant")) == off
        db.close()
