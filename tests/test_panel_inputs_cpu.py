"""The inputs and comparisons of tests/test_gpu_svd_panel.py have teeth, shown without a GPU: the tiling of k_gemm_tn /
k_gemm_tn_reduce and of k_update restated in numpy (tests/helpers/panel_inputs.py) passes the GPU test's own comparison on every
listed shape, and each named mutant of it — the tail loop dropped, the odd last group skipped, row chunks from the fifth on not
added, the column mask ignored, the single-tile reuse of the coefficients applied above 128 basis columns, the column maxima not
cleared — fails it on at least one.  No GPU test calls the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import panel_inputs as pi  # noqa: E402

KINDS = ("exact", "normal")


def _tn_operands(kind, rows, p, cb):
    return pi.matrix(kind, rows, p, 1), pi.matrix(kind, rows, cb, 2)


def _tn_passes(kind, rows, p, cb, mutant):
    if kind == "normal" and not pi.ld_available(rows):
        return True
    A, B = _tn_operands(kind, rows, p, cb)
    Cbuf = pi.gemm_tn_tiled(A, B, p, cb, p + 3, mutant)
    try:
        pi.check_gemm_tn(Cbuf, A, B, p, cb, kind)
    except AssertionError:
        return False
    return True


def test_gemm_tn_restatement_passes_every_shape():
    for rows, p, cb in pi.tn_cases():
        for kind in KINDS:
            assert _tn_passes(kind, rows, p, cb, None), (kind, rows, p, cb)


@pytest.mark.parametrize("mutant", pi.TN_MUTANTS)
def test_gemm_tn_mutant_is_caught(mutant):
    """every mutant fails on at least one listed shape, with the exact and with the rounding inputs alike"""
    cases = [c for c in pi.tn_cases() if c[1] == 17 and c[2] == 17] + [(4097, 33, 8), (1025, 16, 31)]
    for kind in KINDS:
        caught = [c for c in cases if not _tn_passes(kind, *c, mutant)]
        print(mutant, kind, "caught at", caught)
        assert caught, (mutant, kind)


def test_gemm_tn_mutants_bite_where_the_shapes_say():
    """the shapes are in the list for a reason: 33 rows is the first with a tail behind a whole group, 32 the first odd last group,
    9 * 1024 + 300 the only one with a third turn of the reduce loop, and every cb that is no multiple of 16 has masked columns"""
    assert not _tn_passes("exact", 33, 17, 17, "no_tail") and _tn_passes("exact", 32, 17, 17, "no_tail")
    assert not _tn_passes("exact", 32, 17, 17, "odd_last_group_skipped") and _tn_passes("exact", 64, 17, 17, "odd_last_group_skipped")
    assert not _tn_passes("exact", 4097, 17, 17, "chunk_ge_4_not_added") and _tn_passes("exact", 1025, 17, 17, "chunk_ge_4_not_added")
    assert not _tn_passes("exact", 1025, 17, 17, "bval_ignored") and _tn_passes("exact", 1025, 17, 32, "bval_ignored")


def _up_operands(kind, n, p, cb):
    return (pi.matrix(kind, n, p, 3), pi.matrix(kind, p, cb, 4) if p else np.zeros((0, cb)), pi.matrix(kind, cb, cb, 5),
            pi.matrix(kind, n, cb, 6))


def _up_passes(kind, n, p, cb, mutant, with_mx=True):
    if kind == "normal" and not pi.ld_available(max(p, 1)):
        return True
    Q, Cm, Ri, W = _up_operands(kind, n, p, cb)
    mx0 = None
    if with_mx:
        mx0 = np.full(16, pi.CANARY_BITS, dtype=np.uint64)
        mx0[:cb] = 0
    Wbuf, mx = pi.update_tiled(Q, Cm, Ri, W, n + pi.PAD, mx0, mutant)
    try:
        pi.check_update(Wbuf, mx, Q, Cm, Ri, W, kind)
    except AssertionError:
        return False
    return True


def test_update_restatement_passes_every_shape():
    for n, p, cb in pi.update_cases():
        for kind in KINDS:
            assert _up_passes(kind, n, p, cb, None), (kind, n, p, cb)


@pytest.mark.parametrize("mutant", pi.UP_MUTANTS)
def test_update_mutant_is_caught(mutant):
    for kind in KINDS:
        caught = [c for c in pi.update_cases() if not _up_passes(kind, *c, mutant)]
        print(mutant, kind, "caught at", caught)
        assert caught, (mutant, kind)
    if mutant == "one_tile_reuse_above_128":     # 257 rows and 129 columns: the second turn of rows with a second tile
        assert not _up_passes("exact", 257, 129, 9, mutant) and _up_passes("exact", 256, 129, 9, mutant)
        assert _up_passes("exact", 1025, 128, 8, mutant)


def test_update_seeded_maximum_survives_in_the_statement():
    n, p, cb = 257, 1, 7
    Q, Cm, Ri, W = _up_operands("normal", n, p, cb)
    seed = np.zeros(16)
    seed[2] = 1.0e9
    mx0 = np.full(16, pi.CANARY_BITS, dtype=np.uint64)
    mx0[:cb] = seed[:cb].view(np.uint64)
    Wbuf, mx = pi.update_tiled(Q, Cm, Ri, W, n + pi.PAD, mx0)
    pi.check_update(Wbuf, mx, Q, Cm, Ri, W, "normal", mx_seed=seed)
    with pytest.raises(AssertionError):
        pi.check_update(Wbuf, mx, Q, Cm, Ri, W, "normal")


def test_exact_inputs_hold_their_sentinels_and_stay_exact():
    X = pi.exact_matrix(1100, 5, 0)
    for r in (255, 256, 1023, 1024, 1099):
        assert np.all(np.abs(X[r]) == 1000)
    assert np.abs(np.delete(X, [255, 256, 1023, 1024, 1099], axis=0)).max() == 3
    assert np.all(np.abs(pi.exact_matrix(1, 4, 0)) == 1000)
    # a dropped sentinel row changes every entry of the product
    A, B = pi.exact_matrix(300, 3, 1), pi.exact_matrix(300, 2, 2)
    assert np.all(pi.int_matmul(A.T, B) != pi.int_matmul(A[:299].T, B[:299]))


def test_guards():
    P = pi.padded(np.ones((3, 2)))
    assert P.shape == (3 + pi.PAD, 2) and np.all(np.isnan(P[3:])) and np.all(P[:3] == 1)
    Cb = pi.canary(6, 4)
    assert np.all(pi.is_canary(Cb)) and not pi.canary_outside(Cb, 2, 2)
    Cb[:2, :2] = np.nan                         # an ordinary NaN is not the canary
    assert pi.canary_outside(Cb, 2, 2)
    Cb[2, 0] = 0.0
    assert not pi.canary_outside(Cb, 2, 2)


def test_round_cols_statement():
    """ties go to even, the scale is the largest power of two with max * qs <= 0.98 * 2^(8 S - 1), a power-of-two maximum and
    a zero column are handled, rounding twice changes nothing, and a column of ties really is one"""
    for S in range(1, 8):
        X = pi.round_matrix(257, S)
        X[:, 3] = pi.tie_column(257, S, 0)
        R = pi.round_cols_statement(X, S)
        assert pi.bits_equal(pi.round_cols_statement(R, S), R)
        assert np.all(R[:, 1] == 0) and R[:, 2].min() == -0.25 and np.all(R[:, 4] < 0)
        for j in (0, 2, 3, 4, 5):
            m = np.abs(X[:, j]).max()
            e = int(np.frexp(np.ldexp(0.98, 8 * S - 1) / m)[1])
            qs = np.ldexp(1.0, e - 1)
            assert m * qs <= 0.98 * 2.0 ** (8 * S - 1) < 2 * m * qs
            k = R[:, j] * qs
            assert np.all(k == np.rint(k)) and np.abs(k).max() < 2.0 ** (8 * S - 1)
            assert np.abs(R[:, j] - X[:, j]).max() <= 0.5 / qs
        qs = np.ldexp(1.0, int(np.frexp(np.ldexp(0.98, 8 * S - 1))[1]) - 1)
        t = X[1:, 3] * qs
        assert np.all(np.abs(t - np.trunc(t)) == 0.5)                  # on a tie, all of them
        assert np.all(np.rint(t) % 2 == 0) and np.all(R[1:, 3] * qs == np.rint(t))
    assert pi.bits_equal(pi.round_cols_statement(np.array([[-0.001], [1.0]]), 1)[0], np.array([0.0]))      # +0, not -0


def test_fused_twin_flags_the_duplicated_column_only():
    """the CPU twin of the fused step (tests/native/native_test.cpp) on the inputs of the GPU test: no flag and residuals at
    rounding level for the random panel, the flag for the panel with a duplicated column"""
    import build_native
    nt = C.CDLL(build_native.build())
    f64p = C.POINTER(C.c_double)
    nt.nt_fused_orth.restype = C.c_int
    nt.nt_fused_orth.argtypes = [f64p, f64p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, f64p, f64p]
    for nr, p, cb, iters in ((300, 16, 9, 4), (1025, 130, 16, 2), (300, 0, 8, 2)):
        for deficient in (False, True):
            Q, W = pi.fused_input(nr, p, cb, deficient)
            Wn = np.array(W, order="F")
            Qc = np.array(Q, order="F")
            flag, Rout = C.c_double(-1.0), np.zeros((cb, cb), order="F")
            rc = nt.nt_fused_orth(Qc.ctypes.data_as(f64p), Wn.ctypes.data_as(f64p), nr, p, max(p - cb, 0), cb, iters, C.byref(flag),
                                  Rout.ctypes.data_as(f64p))
            if deficient:
                assert rc == -2 and flag.value != 0 and np.array_equal(Wn, W)
                continue
            assert rc == cb and flag.value == 0
            r1, r2, r3 = pi.fused_residuals(Q, W, Wn)
            assert r1 < 1e-13 and r2 < 1e-13 and r3 < (1e-3 if p else 1e-13), (r1, r2, r3)
            if p == 0:      # W = Wn Rout
                assert np.abs(Wn @ Rout - W).max() < 1e-12
    flag, Rout = C.c_double(0), np.zeros(256)
    Q, W = pi.fused_input(400, 369, 16)
    assert nt.nt_fused_orth(np.array(Q, order="F").ctypes.data_as(f64p), np.array(W, order="F").ctypes.data_as(f64p), 400, 369, 353, 16,
                            2, C.byref(flag), Rout.ctypes.data_as(f64p)) == -1
