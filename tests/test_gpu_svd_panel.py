"""The panel kernels of bigsnpr_amd/csrc/svd_panel.hip one at a time, through the bsn_panel_* entries (the launch functions the solve
itself uses), past their tile and loop edges: k_gemm_tn<1|2> + k_gemm_tn_reduce, k_gemm_nn, k_right_mult, k_update<8|16>,
k_col_absmax + k_round_cols, k_take_rows / k_max_over_ranks / k_pack_int / k_unpack_int, k_block / k_unblock / k_place_rows, and
the device queue of the fused block step (k_orth2 between the tall kernels).

Inputs, statements and comparisons: tests/helpers/panel_inputs.py.  Exact inputs (small integers with sentinels of +-1000 in the
rows where chunks, waves and groups end) are compared with np.array_equal against the int64 result; rounding inputs (standard
normal) against the np.longdouble statement within the any-order bound 1.01 k 2^-53 (|A|' |B|) — 1.01 (p + cb + 2) 2^-53
((|W| + |Q| |C|) |Ri|) for k_update, and (p + 2) for k_gemm_nn's alpha In + beta Q S: p products, one rounding of beta * sum, one
of the final sum.  The roundings are compared bit for bit.  Every operand has a leading dimension larger than its row count with
NaN in the padding rows, every output is filled with a canary bit pattern that must survive outside the written region.
tests/test_panel_inputs_cpu.py shows without a GPU that these shapes and comparisons catch a wrong tiling."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import panel_inputs as pi  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = pi.PAD
KINDS = ("exact", "normal")


@pytest.fixture(scope="module")
def lib():
    from bigsnpr_amd import _lib
    return _lib


def _dev(lib, a):
    """a host array (any dtype of 8 bytes, column-major as given) on the device"""
    a = np.asfortranarray(a)
    return lib.DeviceArray.from_numpy(a.view(np.float64) if a.dtype != np.float64 else a)


def _off(d, elems):
    return C.c_void_p(d.ptr.value + 8 * int(elems))


def _refused(lib, rc, text):
    assert rc != 0 and rc != -1
    msg = lib.load().bsn_last_error().decode()
    assert text in msg, msg


def _skip_without_ld(k):
    if not pi.ld_available(k):
        pytest.skip("no extended precision on this platform: rounding inputs with more than 300 rows")


# ---- k_gemm_tn + k_gemm_tn_reduce ---------------------------------------------------------------------------------------------
def _gemm_tn(lib, kind, rows, p, cb, ldc=None):
    L = lib.load()
    A, B = pi.matrix(kind, rows, p, 1), pi.matrix(kind, rows, cb, 2)
    ldc = p + 3 if ldc is None else ldc
    dA, dB, dC = _dev(lib, pi.padded(A)), _dev(lib, pi.padded(B, rows + PAD + 2)), _dev(lib, pi.canary(ldc, 33))
    lib.check(L.bsn_panel_gemm_tn(dA.ptr, rows + PAD, p, dB.ptr, rows + PAD + 2, cb, rows, dC.ptr, ldc))
    got = dC.to_numpy()
    for d in (dA, dB, dC):
        d.free()
    return pi.check_gemm_tn(got, A, B, p, cb, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", pi.TN_ROWS)
def test_gemm_tn_rows(lib, rows, kind):
    """(p, cb) = (17, 17) — two tiles of A, two of B, both ragged — at every row count: nfull = 0 .. 3 and 8, a wave with one
    row, a second chunk of one row, the reduce loop's second (4097) and third (9516) turn.  lda != ldb."""
    if kind == "normal":
        _skip_without_ld(rows)
    print("rows %d %s: error / bound %.3f" % (rows, kind, _gemm_tn(lib, kind, rows, 17, 17)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", pi.TN_PAIR_ROWS)
def test_gemm_tn_columns(lib, rows, kind):
    """every (p, cb) of {1, 15, 16, 17, 33, 400} x {1, 8, 15, 16, 17, 31, 32} at 1025 and 4097 rows"""
    if kind == "normal":
        _skip_without_ld(rows)
    worst = max(_gemm_tn(lib, kind, rows, p, cb) for p in pi.TN_P for cb in pi.TN_CB)
    print("rows %d %s: largest error / bound %.3f" % (rows, kind, worst))


@pytest.mark.parametrize("kind", KINDS)
def test_gemm_tn_gram_alias_and_ldc(lib, kind):
    """B = columns p0 .. of A (the Gram case of QtQ: 16 columns from 17 on, and the 2 cb = 32 of the fused step's X), and C
    with ldc = p + cb as the X block of the fused step"""
    L = lib.load()
    rows, p = 1025, 33
    A = pi.matrix(kind, rows, p, 7)
    ld = rows + PAD
    dA = _dev(lib, pi.padded(A))
    for p0, cb, ldc in ((17, 16, p), (1, 32, p + 16), (32, 1, p + 1)):
        dC = _dev(lib, pi.canary(ldc, 33))
        lib.check(L.bsn_panel_gemm_tn(dA.ptr, ld, p, _off(dA, ld * p0), ld, cb, rows, dC.ptr, ldc))
        pi.check_gemm_tn(dC.to_numpy(), A, A[:, p0:], p, cb, kind)
        dC.free()
    assert pi.bits_equal(dA.to_numpy(), pi.padded(A))      # (the operands are not written)
    dA.free()


def test_gemm_tn_refusals(lib):
    L = lib.load()
    rows, p = 40, 5
    dA, dB, dC = _dev(lib, pi.padded(pi.exact_matrix(rows, p, 1))), _dev(lib, pi.padded(pi.exact_matrix(rows, 33, 2))), _dev(lib, pi.canary(p, 40))
    ld = rows + PAD
    _refused(lib, L.bsn_panel_gemm_tn(dA.ptr, ld, p, dB.ptr, ld, 33, rows, dC.ptr, p), "internal: panel product with 33 columns")
    _refused(lib, L.bsn_panel_gemm_tn(None, ld, p, dB.ptr, ld, 3, rows, dC.ptr, p), "bsn_panel_gemm_tn: null pointer")
    _refused(lib, L.bsn_panel_gemm_tn(dA.ptr, ld, p, None, ld, 3, rows, dC.ptr, p), "bsn_panel_gemm_tn: null pointer")
    _refused(lib, L.bsn_panel_gemm_tn(dA.ptr, ld, p, dB.ptr, ld, 3, rows, None, p), "bsn_panel_gemm_tn: null pointer")
    for args in ((rows - 1, p, ld, 3, rows, p), (ld, p, rows - 1, 3, rows, p), (ld, p, ld, 3, rows, p - 1), (ld, 0, ld, 3, rows, p),
                 (ld, p, ld, 0, rows, p), (ld, p, ld, 3, 0, p)):
        lda, pp, ldb, cb, rr, ldc = args
        _refused(lib, L.bsn_panel_gemm_tn(dA.ptr, lda, pp, dB.ptr, ldb, cb, rr, dC.ptr, ldc), "bsn_panel_gemm_tn: dimensions")
    assert np.all(pi.is_canary(dC.to_numpy()))
    for d in (dA, dB, dC):
        d.free()


# ---- k_gemm_nn ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", pi.NN_N)
def test_gemm_nn(lib, n, kind):
    """p = 1, 255, 256, 257, 513 (the 256-column LDS tile, its second and third turn) x nc = 1, 8, 9, 16, as the call sites run
    it: W <- W - Q C in place (alpha 1, beta -1, Out == In; W_minus_QC) and Out = Q S with In = NULL, alpha 0 (Ritz vectors, u and v,
    thick restart)"""
    L = lib.load()
    ld = n + PAD
    for p in pi.NN_P:
        if kind == "normal":
            _skip_without_ld(p)
        Q = pi.matrix(kind, n, p, 11)
        dQ = _dev(lib, pi.padded(Q))
        for nc in pi.NN_NC:
            S, W = pi.matrix(kind, p, nc, 12), pi.matrix(kind, n, nc, 13)
            dS = _dev(lib, S)
            for alpha, beta, with_in, in_place in pi.NN_MODES:
                buf = pi.canary(ld + 1, nc + 1)
                if in_place:
                    buf[:ld, :nc] = pi.padded(W)
                dO = _dev(lib, buf)
                lib.check(L.bsn_panel_gemm_nn(dQ.ptr, ld, p, dS.ptr, nc, dO.ptr if with_in else None, (ld + 1) if with_in else 0,
                                              alpha, beta, dO.ptr, ld + 1, n))
                got = dO.to_numpy()
                dO.free()
                if in_place:
                    assert np.all(np.isnan(got[n:ld, :nc])) and np.all(pi.is_canary(got[ld:])) and np.all(pi.is_canary(got[:, nc:]))
                else:
                    assert pi.canary_outside(got, n, nc)
                pi.check_product(got[:n, :nc], Q, S, kind, p, base=W if with_in else None, scale=beta, extra=2)
            dS.free()
        dQ.free()


def test_gemm_nn_refusals(lib):
    L = lib.load()
    n, p = 30, 4
    dQ, dS, dO = _dev(lib, pi.exact_matrix(n, p, 1)), _dev(lib, pi.exact_matrix(p, 17, 2)), _dev(lib, pi.canary(n, 17))
    _refused(lib, L.bsn_panel_gemm_nn(dQ.ptr, n, p, dS.ptr, 17, None, 0, 0.0, 1.0, dO.ptr, n, n), "bsn_panel_gemm_nn: dimensions")
    _refused(lib, L.bsn_panel_gemm_nn(dQ.ptr, n, p, dS.ptr, 0, None, 0, 0.0, 1.0, dO.ptr, n, n), "bsn_panel_gemm_nn: dimensions")
    _refused(lib, L.bsn_panel_gemm_nn(dQ.ptr, n - 1, p, dS.ptr, 2, None, 0, 0.0, 1.0, dO.ptr, n, n), "bsn_panel_gemm_nn: dimensions")
    _refused(lib, L.bsn_panel_gemm_nn(dQ.ptr, n, p, dS.ptr, 2, None, 0, 0.0, 1.0, dO.ptr, n - 1, n), "bsn_panel_gemm_nn: dimensions")
    _refused(lib, L.bsn_panel_gemm_nn(dQ.ptr, n, p, dS.ptr, 2, dO.ptr, n - 1, 1.0, 1.0, dO.ptr, n, n), "bsn_panel_gemm_nn: dimensions")
    _refused(lib, L.bsn_panel_gemm_nn(dQ.ptr, n, p, dS.ptr, 2, None, 0, 1.0, 1.0, dO.ptr, n, n), "bsn_panel_gemm_nn: null pointer")
    _refused(lib, L.bsn_panel_gemm_nn(dQ.ptr, n, p, dS.ptr, 2, None, 0, 0.0, 1.0, None, n, n), "bsn_panel_gemm_nn: null pointer")
    assert np.all(pi.is_canary(dO.to_numpy()))
    for d in (dQ, dS, dO):
        d.free()


# ---- k_right_mult ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", pi.RM_N)
def test_right_mult(lib, n, kind):
    """in place W[:, :r] = W[:, :cb] M at (cb, r) = (1, 1), (8, 3), (16, 16), (16, 1), (9, 9); the columns from r on stay"""
    L = lib.load()
    ld = n + PAD
    for cb, r in pi.RM_SHAPES:
        W, M = pi.matrix(kind, n, cb, 21), pi.matrix(kind, cb, r, 22)
        buf = pi.canary(ld, cb + 1)
        buf[:, :cb] = pi.padded(W)
        dW, dM = _dev(lib, buf), _dev(lib, M)
        lib.check(L.bsn_panel_right_mult(dW.ptr, ld, n, cb, r, dM.ptr))
        got = dW.to_numpy()
        dW.free(), dM.free()
        assert np.all(np.isnan(got[n:, :cb])) and np.all(pi.is_canary(got[:, cb:])) and pi.bits_equal(got[:n, r:cb], W[:, r:])
        pi.check_product(got[:n, :r], W, M, kind, cb)


def test_right_mult_refusals(lib):
    L = lib.load()
    n = 20
    dW, dM = _dev(lib, pi.exact_matrix(n, 17, 1)), _dev(lib, pi.exact_matrix(17, 17, 2))
    for cb, r, ld in ((17, 1, n), (1, 17, n), (0, 1, n), (1, 0, n), (4, 4, n - 1)):
        _refused(lib, L.bsn_panel_right_mult(dW.ptr, ld, n, cb, r, dM.ptr), "bsn_panel_right_mult: dimensions")
    _refused(lib, L.bsn_panel_right_mult(None, n, n, 2, 2, dM.ptr), "bsn_panel_right_mult: null pointer")
    _refused(lib, L.bsn_panel_right_mult(dW.ptr, n, n, 2, 2, None), "bsn_panel_right_mult: null pointer")
    dW.free(), dM.free()


# ---- k_update -------------------------------------------------------------------------------------------------------------------
def _mx_buffer(cb, seed=None):
    mx = np.full(16, pi.CANARY_BITS, dtype=np.uint64)
    mx[:cb] = 0 if seed is None else seed[:cb].view(np.uint64)
    return mx


def _update(lib, kind, n, p, cb, with_mx, seed=None):
    L = lib.load()
    ldq, ldw = n + PAD, n + PAD + 2
    Q = pi.matrix(kind, n, p, 3)
    Cm = pi.matrix(kind, p, cb, 4) if p else np.zeros((0, cb))
    Ri, W = pi.matrix(kind, cb, cb, 5), pi.matrix(kind, n, cb, 6)
    buf = pi.canary(ldw, cb + 2)
    buf[:, :cb] = pi.padded(W, ldw)
    dQ = _dev(lib, pi.padded(Q)) if p else None
    dC = _dev(lib, Cm) if p else None
    dRi, dW = _dev(lib, Ri), _dev(lib, buf)
    dmx = _dev(lib, _mx_buffer(cb, seed)) if with_mx else None
    lib.check(L.bsn_panel_update(dQ.ptr if p else None, ldq, p, dC.ptr if p else None, dRi.ptr, cb, dW.ptr, ldw, n,
                                 dmx.ptr if with_mx else None))
    got = dW.to_numpy()
    mx = dmx.to_numpy().view(np.uint64).ravel() if with_mx else None
    for d in (dQ, dC, dRi, dW, dmx):
        if d is not None:
            d.free()
    pi.check_update(got, mx, Q, Cm, Ri, W, kind, mx_seed=seed)
    return got, mx


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_mx", (False, True))
def test_update(lib, with_mx, kind):
    """every n of {1, 255, 256, 257, 1023, 1024, 1025, 2049} at (p, cb) = (129, 9) and (128, 8) — a second coefficient tile
    against a single reused one, both templates — and every (p, cb) of {0, 1, 127, 128, 129, 300} x {1, 7, 8, 9, 15, 16} at
    n = 1025; with the maxima: bit for bit the column maxima of |W| as the same call returned it, mx[cb .. 15] untouched"""
    for n, p, cb in pi.update_cases():
        if kind == "normal":
            _skip_without_ld(max(p, 1))
        _update(lib, kind, n, p, cb, with_mx)


def test_update_seeded_maximum_survives(lib):
    """the maxima are folded in by atomic max: a larger value that is there before the call stays, a smaller one is replaced"""
    for cb in (7, 16):
        seed = np.zeros(16)
        seed[0], seed[cb - 1] = 1.0e9, 2.0 ** -30
        got, mx = _update(lib, "normal", 1025, 129, cb, True, seed)
        assert mx[0] == np.array([1.0e9]).view(np.uint64)[0] and mx[cb - 1] == np.abs(got[:1025, cb - 1]).max().view(np.uint64)


def test_update_refusals(lib):
    L = lib.load()
    n, p = 20, 3
    dQ, dC, dRi, dW = (_dev(lib, pi.exact_matrix(n, p, 1)), _dev(lib, pi.exact_matrix(p, 17, 2)), _dev(lib, pi.exact_matrix(17, 17, 3)),
                       _dev(lib, pi.canary(n, 17)))
    for pp, cb, ldq, ldw in ((p, 17, n, n), (p, 0, n, n), (-1, 2, n, n), (p, 2, n - 1, n), (p, 2, n, n - 1)):
        _refused(lib, L.bsn_panel_update(dQ.ptr, ldq, pp, dC.ptr, dRi.ptr, cb, dW.ptr, ldw, n, None), "bsn_panel_update: dimensions")
    _refused(lib, L.bsn_panel_update(None, n, p, dC.ptr, dRi.ptr, 2, dW.ptr, n, n, None), "bsn_panel_update: null pointer")
    _refused(lib, L.bsn_panel_update(dQ.ptr, n, p, None, dRi.ptr, 2, dW.ptr, n, n, None), "bsn_panel_update: null pointer")
    _refused(lib, L.bsn_panel_update(dQ.ptr, n, p, dC.ptr, None, 2, dW.ptr, n, n, None), "bsn_panel_update: null pointer")
    _refused(lib, L.bsn_panel_update(dQ.ptr, n, p, dC.ptr, dRi.ptr, 2, None, n, n, None), "bsn_panel_update: null pointer")
    assert np.all(pi.is_canary(dW.to_numpy()))
    for d in (dQ, dC, dRi, dW):
        d.free()


# ---- k_col_absmax + k_round_cols ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", pi.ROUND_ROWS)
def test_round_cols(lib, rows):
    """slices 1 .. 7 on a normal column, a zero column (stays an unscaled zero), a power-of-two maximum, a column with every entry
    on a rounding tie, a negative column and a tiny one; the 256- and the 64-workgroup form of k_col_absmax (their grid-stride
    loops take a second turn from 262 145 and 65 537 rows); bit for bit, and the maxima bit for bit too"""
    L = lib.load()
    ld = rows + PAD
    for S in range(1, 8):
        X = pi.round_matrix(rows, S)
        X[:, 3] = pi.tie_column(rows, S, 0)
        want = pi.round_cols_statement(X, S)
        cb = X.shape[1]
        buf = pi.canary(ld, cb + 1)
        buf[:, :cb] = pi.padded(X)
        for wide in (1, 0):
            dX, dmx = _dev(lib, buf), _dev(lib, np.full(16, pi.CANARY_BITS, dtype=np.uint64))
            lib.check(L.bsn_panel_round_cols(dX.ptr, ld, rows, cb, S, 0, dmx.ptr, wide))
            got, mx = dX.to_numpy(), dmx.to_numpy().view(np.uint64).ravel()
            dX.free(), dmx.free()
            assert np.all(np.isnan(got[rows:, :cb])) and np.all(pi.is_canary(got[:, cb:])), (S, wide)
            assert np.array_equal(mx[:cb], np.abs(X).max(axis=0).view(np.uint64)) and np.all(mx[cb:] == pi.CANARY_BITS), (S, wide)
            assert pi.bits_equal(got[:rows, :cb], want), (S, wide, np.argwhere(got[:rows, :cb] != want)[:4].tolist())


def test_round_cols_with_the_maxima_of_an_update(lib):
    """have_mx: the maxima come from a preceding k_update (here W <- W I, p = 0, which returns W itself) and k_col_absmax does
    not run; the rounding is that of the whole column"""
    L = lib.load()
    n, cb, S = 2049, 9, 2
    ld = n + PAD
    W = pi.normal_matrix(n, cb, 31)
    W[:, 4] = 0.0
    buf = pi.canary(ld, cb + 1)
    buf[:, :cb] = pi.padded(W)
    dW, dRi, dmx = _dev(lib, buf), _dev(lib, np.eye(cb)), _dev(lib, _mx_buffer(cb))
    lib.check(L.bsn_panel_update(None, 0, 0, None, dRi.ptr, cb, dW.ptr, ld, n, dmx.ptr))
    assert pi.bits_equal(dW.to_numpy()[:n, :cb], W)
    lib.check(L.bsn_panel_round_cols(dW.ptr, ld, n, cb, S, 1, dmx.ptr, 1))
    got, mx = dW.to_numpy(), dmx.to_numpy().view(np.uint64).ravel()
    for d in (dW, dRi, dmx):
        d.free()
    assert np.array_equal(mx[:cb], np.abs(W).max(axis=0).view(np.uint64)) and np.all(mx[cb:] == pi.CANARY_BITS)
    assert np.all(np.isnan(got[n:, :cb])) and np.all(pi.is_canary(got[:, cb:]))
    assert pi.bits_equal(got[:n, :cb], pi.round_cols_statement(W, S))


def test_round_cols_refusals(lib):
    L = lib.load()
    n = 20
    dX, dmx = _dev(lib, pi.exact_matrix(n, 17, 1)), _dev(lib, np.zeros(16))
    for ld, cb, S in ((n - 1, 2, 2), (n, 17, 2), (n, 0, 2), (n, 2, 0), (n, 2, 8)):
        _refused(lib, L.bsn_panel_round_cols(dX.ptr, ld, n, cb, S, 0, dmx.ptr, 1), "bsn_panel_round_cols: dimensions")
    _refused(lib, L.bsn_panel_round_cols(None, n, n, 2, 2, 0, dmx.ptr, 1), "bsn_panel_round_cols: null pointer")
    _refused(lib, L.bsn_panel_round_cols(dX.ptr, n, n, 2, 2, 0, None, 1), "bsn_panel_round_cols: null pointer")
    dX.free(), dmx.free()


# ---- the exchanges of the sharded solve on one device ---------------------------------------------------------------------------
def _block_rows(n, world):
    return ((n + world - 1) // world + 3) // 4 * 4


@pytest.mark.parametrize("n,world", pi.GATHER_CASES)
def test_compact_gather_equals_round_cols(lib, n, world):
    """k_take_rows + k_col_absmax (64 workgroups) per sample block, k_max_over_ranks, k_pack_int<int16 | int32> per block and
    k_unpack_int give the rounding of the whole matrix bit for bit, as the comment in round_W claims: world 1, 2, 3, 8; a last
    block that is partly padding (1000 rows in 3 blocks of 336) and blocks that are wholly padding (17 rows in 8 blocks of 4);
    slices 1, 2 (int16) and 3, 4 (int32)"""
    L = lib.load()
    X = pi.round_matrix(n, world)
    cb = X.shape[1]
    dX = _dev(lib, X)
    for S in (1, 2, 3, 4):
        out = np.full(n * cb + 8, pi.CANARY)
        dO = _dev(lib, out)
        lib.check(L.bsn_panel_compact_gather(dX.ptr, n, cb, world, S, dO.ptr))
        got = dO.to_numpy().ravel()
        dO.free()
        assert np.all(pi.is_canary(got[n * cb:])), (S,)
        got = got[:n * cb].reshape((n, cb), order="F")
        want = pi.round_cols_statement(X, S)
        assert pi.bits_equal(got, want), (S, np.argwhere(got != want)[:4].tolist())
    assert pi.bits_equal(dX.to_numpy(), X)
    dX.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,world", pi.GATHER_CASES)
def test_block_roundtrip_is_the_identity(lib, n, world, kind):
    """k_block then k_unblock is the identity, and k_place_rows of every block rebuilds the matrix with zero rows behind it"""
    L = lib.load()
    for cb in (1, 16):
        X = pi.matrix(kind, n, cb, 41)
        nr = _block_rows(n, world)
        dX, dO, dP = _dev(lib, X), _dev(lib, np.full(n * cb + 8, pi.CANARY)), _dev(lib, np.full(world * nr * cb + 8, pi.CANARY))
        lib.check(L.bsn_panel_block_roundtrip(dX.ptr, n, cb, world, dO.ptr, dP.ptr))
        got, placed = dO.to_numpy().ravel(), dP.to_numpy().ravel()
        for d in (dX, dO, dP):
            d.free()
        assert np.all(pi.is_canary(got[n * cb:])) and np.all(pi.is_canary(placed[world * nr * cb:]))
        assert pi.bits_equal(got[:n * cb].reshape((n, cb), order="F"), X)
        want = np.zeros((world * nr, cb), order="F")
        want[:n] = X
        assert pi.bits_equal(placed[:world * nr * cb].reshape((world * nr, cb), order="F"), want)


def test_exchange_refusals(lib):
    L = lib.load()
    n = 20
    dX, dO = _dev(lib, pi.exact_matrix(n, 17, 1)), _dev(lib, pi.canary(4 * n, 17))
    for cb, world, S in ((17, 2, 2), (0, 2, 2), (2, 0, 2), (2, 65, 2), (2, 2, 0), (2, 2, 5)):
        _refused(lib, L.bsn_panel_compact_gather(dX.ptr, n, cb, world, S, dO.ptr), "bsn_panel_compact_gather: dimensions")
    _refused(lib, L.bsn_panel_compact_gather(None, n, 2, 2, 2, dO.ptr), "bsn_panel_compact_gather: null pointer")
    _refused(lib, L.bsn_panel_compact_gather(dX.ptr, n, 2, 2, 2, None), "bsn_panel_compact_gather: null pointer")
    for cb, world in ((17, 2), (0, 2), (2, 0), (2, 65)):
        _refused(lib, L.bsn_panel_block_roundtrip(dX.ptr, n, cb, world, dO.ptr, dO.ptr), "bsn_panel_block_roundtrip: dimensions")
    _refused(lib, L.bsn_panel_block_roundtrip(dX.ptr, n, 2, 2, dO.ptr, None), "bsn_panel_block_roundtrip: null pointer")
    assert np.all(pi.is_canary(dO.to_numpy()))
    dX.free(), dO.free()


# ---- the fused block step -------------------------------------------------------------------------------------------------------
# Residuals of the device against the same residuals of the CPU twin (tests/native/native_test.cpp, nt_fused_orth: the same
# small-matrix code, plain host loops for the tall products) on the same input; the two sum in different orders, so the cap is a
# ratio: device / max(twin, nr 2^-53).  FUSED_OBSERVED: the largest ratios over all cases of this file on an MI355X, per residual
# max|Wn'Wn - I| (0.0366 at nr 300, p 0, cb 16: device 1.22e-15, twin 1.68e-15, both below the floor nr 2^-53 = 3.3e-14),
# max|Q'Wn| (0.00384 at nr 300, p 130, cb 16, iters 4: device 1.28e-16, twin 8.2e-17) and
# max|(I - Wn Wn')(I - QQ')W| / max|W| (1.00 wherever p > 0: 3e-7 .. 3e-5 on both sides, the distance of the rounded Q from
# an orthonormal basis; 0.03 at p = 0).  The cap is twice the observed ratio, never above 16.
FUSED_OBSERVED = (0.0367, 0.00385, 1.0)
FUSED_CAP = tuple(min(16.0, 2.0 * r) for r in FUSED_OBSERVED)


@pytest.fixture(scope="module")
def twin():
    import build_native
    nt = C.CDLL(build_native.build())
    f64p = C.POINTER(C.c_double)
    nt.nt_fused_orth.restype = C.c_int
    nt.nt_fused_orth.argtypes = [f64p, f64p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, f64p, f64p]

    def run(Q, W, p0, iters):
        nr, cb = W.shape
        Qc, Wn = np.array(Q, order="F"), np.array(W, order="F")
        flag, Rout = C.c_double(-1.0), np.zeros((cb, cb), order="F")
        rc = nt.nt_fused_orth(Qc.ctypes.data_as(f64p), Wn.ctypes.data_as(f64p), nr, Q.shape[1], p0, cb, iters, C.byref(flag),
                              Rout.ctypes.data_as(f64p))
        return rc, flag.value, Wn, Rout
    return run


def _fused_device(lib, Q, W, iters):
    L = lib.load()
    nr, cb = W.shape
    p = Q.shape[1]
    buf = pi.canary(nr, p + cb + 1)
    buf[:, :p], buf[:, p:p + cb] = Q, W
    d = _dev(lib, buf)
    flag, Rout = np.full(1, -1.0), np.full((cb, cb), np.nan, order="F")
    rc = L.bsn_panel_fused_orth(d.ptr, nr, p, max(p - cb, 0), cb, iters, lib.ptr(flag, lib.f64p), lib.ptr(Rout, lib.f64p))
    got = d.to_numpy()
    d.free()
    if rc not in (0, -1):
        lib.check(rc)
    assert pi.bits_equal(got[:, :p], Q) and np.all(pi.is_canary(got[:, p + cb:])), "the fused step wrote outside the panel"
    return rc, flag[0], got[:, p:p + cb], Rout


@pytest.mark.parametrize("nr,p,cb,iters", pi.fused_cases())
def test_fused_step_against_the_cpu_twin(lib, twin, nr, p, cb, iters):
    """gemm_tn -> k_orth2 -> k_update twice, with the [Q W]'[Qb W] product of pass 0 for p > 0, on Q from a QR rounded to the 16-bit
    grid and a random normal panel: no flag on either side, and the three residuals within FUSED_CAP of the twin's"""
    if not pi.HAVE_LD:
        pytest.skip("no extended precision on this platform: the residuals need it")
    Q, W = pi.fused_input(nr, p, cb)
    rc, flag, Wn, Rout = _fused_device(lib, Q, W, iters)
    trc, tflag, tWn, tRout = twin(Q, W, max(p - cb, 0), iters)
    assert rc == 0 and flag == 0.0 and trc == cb and tflag == 0.0, (rc, flag, trc, tflag)
    dev, ref = pi.fused_residuals(Q, W, Wn), pi.fused_residuals(Q, W, tWn)
    ratios = [d / max(t, nr * pi.U) for d, t in zip(dev, ref)]
    print("fused nr %d p %d cb %d iters %d: device %.2e %.2e %.2e twin %.2e %.2e %.2e ratios %.4f %.5f %.4f"
          % ((nr, p, cb, iters) + dev + ref + tuple(ratios)))
    for r, cap in zip(ratios, FUSED_CAP):
        assert r <= cap, (ratios, FUSED_CAP)


@pytest.mark.parametrize("nr,p,cb,iters", [(1025, 0, 8, 2), (1025, 16, 9, 2), (1025, 130, 16, 4), (300, 130, 2, 2), (5000, 368, 16, 2)])
def test_fused_step_flags_a_duplicated_column(lib, twin, nr, p, cb, iters):
    """a panel whose last column repeats its first is rank deficient: the flag is raised on the device and in the twin alike"""
    Q, W = pi.fused_input(nr, p, cb, True)
    rc, flag, Wn, Rout = _fused_device(lib, Q, W, iters)
    trc, tflag, _, _ = twin(Q, W, max(p - cb, 0), iters)
    assert rc == 0 and flag != 0.0 and trc == -2 and tflag != 0.0, (rc, flag, trc, tflag)
    assert np.all(np.isfinite(Wn))       # (the tall kernels stay finite when the step is going to be redone)


def test_fused_step_limits_and_refusals(lib, twin):
    """p + cb = 384 is served (368 + 16 above), 385 and cb = 17 return -1 before anything is launched, as in the twin"""
    L = lib.load()
    nr = 8
    d = _dev(lib, pi.canary(nr, 390))
    flag, Rout = np.full(1, -1.0), np.full(17 * 17, np.nan)
    f, r = lib.ptr(flag, lib.f64p), lib.ptr(Rout, lib.f64p)
    assert L.bsn_panel_fused_orth(d.ptr, nr, 369, 353, 16, 2, f, r) == -1
    assert L.bsn_panel_fused_orth(d.ptr, nr, 17, 0, 17, 2, f, r) == -1
    Q, W = pi.fused_input(400, 369, 16)
    assert twin(Q, W, 353, 2)[0] == -1
    _refused(lib, L.bsn_panel_fused_orth(None, nr, 4, 2, 2, 2, f, r), "bsn_panel_fused_orth: null pointer")
    _refused(lib, L.bsn_panel_fused_orth(d.ptr, nr, 4, 2, 2, 2, None, r), "bsn_panel_fused_orth: null pointer")
    _refused(lib, L.bsn_panel_fused_orth(d.ptr, nr, 4, 2, 2, 2, f, None), "bsn_panel_fused_orth: null pointer")
    _refused(lib, L.bsn_panel_fused_orth(d.ptr, 0, 4, 2, 2, 2, f, r), "bsn_panel_fused_orth: dimensions")
    _refused(lib, L.bsn_panel_fused_orth(d.ptr, nr, 4, 2, 0, 2, f, r), "bsn_panel_fused_orth: dimensions")
    _refused(lib, L.bsn_panel_fused_orth(d.ptr, nr, -1, 0, 2, 2, f, r), "bsn_panel_fused_orth: dimensions")
    _refused(lib, L.bsn_panel_fused_orth(d.ptr, nr, 4, 1, 2, 2, f, r), "bsn_panel_fused_orth: p0 must be p - cb")
    _refused(lib, L.bsn_panel_fused_orth(d.ptr, nr, 0, 1, 2, 2, f, r), "bsn_panel_fused_orth: p0 must be p - cb")
    assert np.all(pi.is_canary(d.to_numpy())) and flag[0] == -1.0
    d.free()
