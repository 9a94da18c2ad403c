"""snp_readBGEN / snp_prodBGEN where the loops of bigsnpr_amd/csrc/bgen.hip go round again: the second
turn of k_bgen_prod over kProdRows rows of Y, its read_as = "random" branch tied to snp_readBGEN's draws across block
sizes and files, ncol at whole tiles and at the grid's limit, the stride of k_bgen_grid8, the refusal of a sample whose
probabilities add up to more than 1, the host walk past the end of a file, and one workgroup of k_inflate that takes
streams with different dynamic tables in turn.  The files are those of tests/helpers/bgen_cases.py, whose conditions
tests/test_bgen_cpu.py proves without a GPU.  Everything is an equality except the dosage product, which keeps the bound
of tests/test_gpu_bgen.py (bgen_cases.check_product)."""
import ctypes as C
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
from test_gpu_bgen import device_inflate, last_ms  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    return bigsnpr_amd


@pytest.fixture(scope="module")
def ab(tmp_path_factory):
    """the file of A and B and its dosages through Python's zlib (computed once, left unchanged)"""
    f = bc.case_ab(tmp_path_factory.mktemp("ab"))
    _, f["X"], _, _ = bi.decode_file(f["path"], f["offs"])
    return f


def dosage_of(ba, fbm_bytes):
    return ba.CODE_DOSAGE[fbm_bytes]


def random_want(f, rows, seed, col0=0):
    out = np.empty((len(rows), f["K"]), dtype=np.uint8)
    for j, block in enumerate(bc.blocks(f)):
        out[:, j], _ = ref.variant(block, f["N"], rows, bi.DECODE_BYTES, 0, seed, col0 + j)
    return out


def exact_product(X, beta):
    """X beta over small integers (every partial sum is an integer below 2^53: any order gives these bits), NaN rows kept"""
    nan_row = np.isnan(X).any(axis=1)
    want = np.nan_to_num(X) @ beta
    want[nan_row] = np.nan
    return want, nan_row


# ---- A: the second turn of k_bgen_prod's loop over rows of Y -------------------------------------------------------------------
@pytest.mark.parametrize("block_size", [1000, 129, 256])
@pytest.mark.parametrize("ncol", [8, 9, 16])
def test_A_product_second_turn(ba, ab, ncol, block_size):
    beta = np.random.default_rng(100 * ncol + block_size).standard_normal((ab["K"], ncol))
    got = ba.snp_prodBGEN(ab["path"], beta, [ab["ids"]], block_size=block_size)
    bc.check_product(got, ab["X"], beta)
    assert np.array_equal(np.isnan(got).any(axis=1), ab["miss"].any(axis=1))
    ms = last_ms(ba)
    assert ms[0] > 0 and ms[1] == 0 and ms[2] > 0


# ---- B: random calls in the product are those of snp_readBGEN ---------------------------------------------------------------------
def test_B_random_product_equals_the_read_draws(ba, ab):
    rows, s, beta = ab["rows_B"], ab["seed"], ab["beta_B"]
    res = ba.snp_readBGEN(ab["path"], [ab["ids"]], ind_row=rows, read_as="random", seed=s, return_bytes=True)
    assert np.array_equal(res.bytes, random_want(ab, rows, s))
    X = dosage_of(ba, res.bytes)
    want, nan_row = exact_product(X, beta)
    assert 0 < nan_row.sum() < rows.size and np.array_equal(nan_row, ab["miss"][rows].any(axis=1))
    got = [ba.snp_prodBGEN(ab["path"], beta, [ab["ids"]], ind_row=rows, read_as="random", seed=s, block_size=b)
           for b in ab["block_sizes_B"]]
    for g in got:
        assert g.shape == want.shape and np.array_equal(g, want, equal_nan=True)
        assert np.array_equal(np.isnan(g), np.repeat(nan_row[:, None], beta.shape[1], axis=1))
    other = ba.snp_prodBGEN(ab["path"], beta, [ab["ids"]], ind_row=rows, read_as="random", seed=s + 1)
    assert not np.array_equal(other, want, equal_nan=True)


# ---- C: three files, the third with a second turn at col0 = 6 ------------------------------------------------------------------------
def test_C_random_product_over_three_files(ba, tmp_path):
    c = bc.case_c(tmp_path)
    files, ids = [f["path"] for f in c["files"]], [f["ids"] for f in c["files"]]
    res = ba.snp_readBGEN(files, ids, ind_row=c["rows"], read_as="random", seed=c["seed"], return_bytes=True)
    col0 = np.cumsum([0] + [f["K"] for f in c["files"]])
    assert np.array_equal(res.bytes, np.concatenate([random_want(f, c["rows"], c["seed"], col0[k])
                                                     for k, f in enumerate(c["files"])], axis=1))
    want, nan_row = exact_product(dosage_of(ba, res.bytes), c["beta"])
    assert 0 < nan_row.sum() < c["rows"].size
    got = ba.snp_prodBGEN(files, c["beta"], ids, ind_row=c["rows"], read_as="random", seed=c["seed"],
                          block_size=c["block_size"])
    assert np.array_equal(got, want, equal_nan=True)
    # and in dosage mode the same three files against the decode, to the bound
    X = np.concatenate([bi.decode_file(f["path"], f["offs"], c["rows"])[1] for f in c["files"]], axis=1)
    beta = np.random.default_rng(36).standard_normal(c["beta"].shape)
    bc.check_product(ba.snp_prodBGEN(files, beta, ids, ind_row=c["rows"]), X, beta)


# ---- D: the stride of k_bgen_grid8 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("read_as", ["dosage", "random"])
def test_D_more_rows_than_threads(ba, tmp_path, read_as):
    f = bc.case_d(tmp_path)
    rows = f["rows"]
    res = ba.snp_readBGEN(f["path"], [f["ids"]], ind_row=rows, read_as=read_as, seed=f["seed"], return_bytes=True)
    want_dos, _, _, sums = bi.decode_file(f["path"], f["offs"], rows)
    want = want_dos if read_as == "dosage" else random_want(f, rows, f["seed"])
    assert res.bytes.shape == want.shape == (rows.size, 3) and np.array_equal(res.bytes, want)
    assert np.array_equal(res.bytes[bc.GRID8_THREADS:], want[bc.GRID8_THREADS:])            # (the second turn by itself)
    info, freq = bi.info_freq(sums)
    assert np.array_equal(res.map["info"], info, equal_nan=True) and np.array_equal(res.map["freq"], freq, equal_nan=True)
    twin = ba.FBM_code256(res.bytes, ba.CODE_DOSAGE)
    assert res._has_na == twin._has_na == bool((want == 3).any()) and res._has_na
    a, b = ba.snp_colstats(res), ba.snp_colstats(twin)
    np.testing.assert_array_equal(a["sumX"], b["sumX"])
    np.testing.assert_array_equal(a["denoX"], b["denoX"])


# ---- E: a sample whose probabilities add up to more than 1 -----------------------------------------------------------------------
MORE_THAN_1 = "add up to more than 1"


def read_is_right(ba, f, rows=None, **kw):
    res = ba.snp_readBGEN(f["path"], [f["ids"]], ind_row=rows, return_bytes=True, **kw)
    want, X, _, sums = bi.decode_file(f["path"], f["offs"], rows)
    assert np.array_equal(res.bytes, want)
    info, freq = bi.info_freq(sums)
    assert np.array_equal(res.map["info"], info, equal_nan=True) and np.array_equal(res.map["freq"], freq, equal_nan=True)
    return X


def test_E_refusal_at_511_and_not_at_510(ba, tmp_path):
    e = bc.case_e(tmp_path)
    good, bad, bv = e["good"], e["bad"], e["block"]
    beta = np.random.default_rng(37).standard_normal((7, 3))
    X = read_is_right(ba, good, block_variants=bv)
    assert X[e["sample"], e["variant"]] == 0.0                      # 2 p0 + p1 = 510: the table's last entry
    bc.check_product(ba.snp_prodBGEN(good["path"], beta, [good["ids"]], block_size=bv), X, beta)
    with pytest.raises(ba.BsnError, match=MORE_THAN_1):
        ba.snp_readBGEN(bad["path"], [bad["ids"]], block_variants=bv)
    with pytest.raises(ba.BsnError, match=MORE_THAN_1):
        ba.snp_prodBGEN(bad["path"], beta, [bad["ids"]], block_size=bv)
    # without the sample the same file is read and multiplied
    rows = e["without"]
    X = read_is_right(ba, bad, rows, block_variants=bv)
    bc.check_product(ba.snp_prodBGEN(bad["path"], beta, [bad["ids"]], ind_row=rows, block_size=bv), X, beta)
    # the variant by itself is refused too, and the others by themselves are not
    with pytest.raises(ba.BsnError, match=MORE_THAN_1):
        ba.snp_readBGEN(bad["path"], [[bad["ids"][e["variant"]]]])
    others = [j for j in range(7) if j != e["variant"]]
    res = ba.snp_readBGEN(bad["path"], [[bad["ids"][j] for j in others]], return_bytes=True)
    assert np.array_equal(res.bytes, bi.decode_file(bad["path"], [bad["offs"][j] for j in others])[0])
    read_is_right(ba, good)


def test_E_refusal_in_the_third_file_frees_the_image(ba, tmp_path, monkeypatch):
    e3 = bc.case_e_files(tmp_path)
    files, ids = [f["path"] for f in e3["bad"]], [f["ids"] for f in e3["bad"]]
    import bigsnpr_amd.bgen as host
    real = host._lib.load()
    made, closed = [], []

    class Spy:
        """the library, with the image handles bsn_bgen_read leaves behind and those bsn_bed_close gets written down"""
        def __getattr__(self, name):
            return getattr(real, name)

        def bsn_bgen_read(self, *a):
            rc = real.bsn_bgen_read(*a)
            made.append(a[12]._obj.value)
            return rc

        def bsn_bed_close(self, h):
            closed.append(h.value)
            return real.bsn_bed_close(h)

    monkeypatch.setattr(host._lib, "load", lambda: Spy())
    with pytest.raises(ba.BsnError, match=MORE_THAN_1):
        ba.snp_readBGEN(files, ids, return_bytes=True)
    monkeypatch.undo()
    assert len(made) == 3 and made[0] and made[0] == made[1] == made[2]      # one image, made by the first file's call
    assert closed == [made[0]]                                                 # and closed once
    with pytest.raises(ba.BsnError, match=MORE_THAN_1):
        ba.snp_prodBGEN(files, np.ones(12), ids)
    # the same call on the control files works
    files, ids = [f["path"] for f in e3["good"]], [f["ids"] for f in e3["good"]]
    res = ba.snp_readBGEN(files, ids, return_bytes=True)
    parts = [bi.decode_file(f["path"], f["offs"]) for f in e3["good"]]
    assert np.array_equal(res.bytes, np.concatenate([p[0] for p in parts], axis=1))
    beta = np.random.default_rng(38).standard_normal(12)
    bc.check_product(ba.snp_prodBGEN(files, beta, ids), np.concatenate([p[1] for p in parts], axis=1), beta)


# ---- F: the grid's y at its limit --------------------------------------------------------------------------------------------------
def test_F_as_many_columns_as_the_grid_takes(ba, tmp_path):
    f = bc.case_f(tmp_path)
    x = bi.DECODE_DOSAGE[2 * int(f["p0"][0, 0]) + int(f["p1"][0, 0])]
    beta = np.random.default_rng(39).standard_normal((1, f["ncol"] + 1))
    got = ba.snp_prodBGEN(f["path"], beta[:, :f["ncol"]], [f["ids"]])
    assert got.shape == (1, 65535 * 8) and np.array_equal(got, x * beta[:, :f["ncol"]])   # one product per entry: exact
    with pytest.raises(ba.BsnError, match="too many columns in 'beta'"):
        ba.snp_prodBGEN(f["path"], beta, [f["ids"]])
    assert np.array_equal(ba.snp_prodBGEN(f["path"], beta[:, :9], [f["ids"]]), x * beta[:, :9])


# ---- G: the host walk past the end of the file ----------------------------------------------------------------------------------------
def test_G_records_past_the_end_of_the_file(ba, tmp_path):
    g = bc.case_g(tmp_path)
    past = r"A variant's record runs past the end of the file\."
    for path in [g["cut"]] + [p for p, _ in g["moved"].values()]:
        with pytest.raises(ba.BsnError, match=past):
            ba.snp_readBGEN(path, [g["ids"]])
        with pytest.raises(ba.BsnError, match=past):
            ba.snp_prodBGEN(path, np.ones(g["K"]), [g["ids"]])
        with pytest.raises(ba.BsnError, match=past):
            ba.snp_readBGEN(path, [g["ids"]], block_variants=1)       # after three good blocks
        X = read_is_right(ba, g)
        beta = np.random.default_rng(40).standard_normal(g["K"])
        bc.check_product(ba.snp_prodBGEN(g["path"], beta, [g["ids"]]), X, beta)
    # the records before the cut are read from the cut file as from the whole one
    res = ba.snp_readBGEN(g["cut"], [g["ids"][:-1]], return_bytes=True)
    assert np.array_equal(res.bytes, bi.decode_file(g["path"], g["offs"][:-1])[0])


# ---- one workgroup of k_inflate, streams with different dynamic tables in turn ------------------------------------------------------
def test_inflate_rebuilds_its_tables_between_streams(ba):
    """2 x (compute units x 4) + 1 streams: k_inflate is launched with compute units x 4 workgroups, so each takes two
    streams and the first takes three; stream k is dyn_lit15 or dyn_two_tables by the parity of k + k // workgroups, so a
    workgroup's next stream is always the other kind, whose tables it builds in LDS over those of the last one"""
    hip = C.CDLL("libamdhip64.so")
    cus = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(cus), 63, 0) == 0 and 0 < cus.value <= 4096   # hipDeviceAttributeMultiprocessorCount
    groups = cus.value * 4
    by = {c[0]: c for c in bi.corpus()}
    kinds = [by["dyn_lit15"], by["dyn_two_tables"]]
    pick = [kinds[(k + k // groups) % 2] for k in range(2 * groups + 1)]
    assert all(pick[k] is not pick[k + groups] for k in range(groups + 1))
    out, status, want_out, want_status, off = device_inflate(ba, [c[1] for c in pick], [len(c[2]) for c in pick])
    assert not status.any() and not want_status.any()
    assert np.array_equal(out, want_out)
    assert out.tobytes() == b"".join(c[2] for c in pick)
