"""Inputs, statements and comparisons of tests/test_gpu_svd_panel.py (the panel kernels of bigsnpr_amd/csrc/svd_panel.hip reached
through the bsn_panel_* entries), plain numpy, seeded, no GPU.  tests/test_panel_inputs_cpu.py shows without a GPU that the
listed shapes have teeth: the tiling of k_gemm_tn / k_gemm_tn_reduce and of k_update restated here passes every comparison,
and each named mutant of it fails at least one.

* exact inputs: small integers (-3 .. 3) stored as doubles with sentinels of +-1000 in the last row and in rows 255, 256, 1023
  and 1024: every sum stays far below 2^53, so the int64 numpy result is THE result whatever the order or fusing, compared
  with np.array_equal;
* rounding inputs: standard normal entries, the statement in np.longdouble, the any-order bound gamma_k entrywise:
  1.01 k 2^-53 (|A|' |B|) for a sum of k products (an FMA is no worse);
* guards: leading dimensions larger than the row count with NaN in the padding rows, output buffers filled with a canary bit
  pattern that must survive wherever the kernel has no business writing.
Nothing here imports bigsnpr_amd."""
import functools
from fractions import Fraction

import numpy as np

LD = np.longdouble
HAVE_LD = np.finfo(LD).nmant >= 63          # x87 extended or better; otherwise Fractions on the shapes with <= 300 rows
U = 2.0 ** -53
PAD = 5                                      # padding rows of every operand (odd: the 16-byte loads of k_gemm_tn get 8-byte columns)
CANARY_BITS = np.uint64(0x7FF8C0DEC0DEC0DE)  # a quiet NaN with a payload no arithmetic produces
CANARY = np.array([CANARY_BITS], dtype=np.uint64).view(np.float64)[0]
SENTINEL_ROWS = (255, 256, 1023, 1024)

# ---- the shapes of the issue -----------------------------------------------------------------------------------------------
TN_ROWS = (1, 7, 8, 9, 31, 32, 33, 64, 96, 255, 256, 257, 1023, 1024, 1025, 4 * 1024 + 1, 9 * 1024 + 300)
TN_P = (1, 15, 16, 17, 33, 400)
TN_CB = (1, 8, 15, 16, 17, 31, 32)
TN_PAIR_ROWS = (1025, 4 * 1024 + 1)


def tn_cases():
    """(rows, p, cb): every rows with (17, 17), every (p, cb) pair with rows = 1025 and 4097"""
    out = [(r, 17, 17) for r in TN_ROWS]
    out += [(r, p, cb) for r in TN_PAIR_ROWS for p in TN_P for cb in TN_CB if (r, p, cb) not in out]
    return out


NN_P = (1, 255, 256, 257, 513)
NN_NC = (1, 8, 9, 16)
NN_N = (1, 255, 256, 257, 1000)
# (alpha, beta, In given, in place): W_minus_QC (W <- W - Q C in place) and the Ritz / u, v / restart formation (Out = Q S)
NN_MODES = ((1.0, -1.0, True, True), (0.0, 1.0, False, False))
RM_SHAPES = ((1, 1), (8, 3), (16, 16), (16, 1), (9, 9))
RM_N = (1, 255, 256, 257)
UP_CB = (1, 7, 8, 9, 15, 16)
UP_P = (0, 1, 127, 128, 129, 300)
UP_N = (1, 255, 256, 257, 1023, 1024, 1025, 2049)


def update_cases():
    """(n, p, cb): every n with (129, 9) and (128, 8), every (p, cb) pair with n = 1025"""
    out = [(n, 129, 9) for n in UP_N] + [(n, 128, 8) for n in UP_N]
    out += [(1025, p, cb) for p in UP_P for cb in UP_CB if (1025, p, cb) not in out]
    return out


ROUND_ROWS = (1, 257, 65537, 262145)
GATHER_CASES = ((1000, 1), (1000, 2), (1000, 3), (1000, 8), (17, 8), (17, 3), (4, 1))   # (n, world)
# (nr, p, cb, iters) of the fused step: every (p, cb) with nr = 1025, the extremes with 300 and 5000 rows and with iters = 4
FUSED_P = (0, 16, 130, 368)
FUSED_CB = (1, 8, 9, 16)


def fused_cases():
    out = [(1025, p, cb, 2) for p in FUSED_P for cb in FUSED_CB]
    out += [(300, 0, 16, 2), (300, 16, 9, 4), (300, 130, 8, 2), (300, 130, 16, 4), (5000, 0, 1, 4), (5000, 16, 16, 2),
            (5000, 130, 9, 2), (5000, 368, 16, 2), (5000, 368, 8, 4), (1025, 368, 16, 4), (1025, 0, 16, 4)]
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def exact_matrix(rows, cols, seed):
    """integers -3 .. 3 as doubles; the last row and rows 255, 256, 1023, 1024 (where they exist) hold +-1000"""
    rng = np.random.default_rng([71, seed, rows, cols])
    X = rng.integers(-3, 4, size=(rows, cols)).astype(np.float64)
    for r in set(SENTINEL_ROWS + (rows - 1,)):
        if 0 <= r < rows:
            X[r, :] = 1000.0 * np.where((np.arange(cols) + r) % 2 == 0, 1.0, -1.0)
    return np.asfortranarray(X)


def normal_matrix(rows, cols, seed):
    return np.asfortranarray(np.random.default_rng([72, seed, rows, cols]).standard_normal((rows, cols)))


def matrix(kind, rows, cols, seed):
    return exact_matrix(rows, cols, seed) if kind == "exact" else normal_matrix(rows, cols, seed)


def padded(X, ld=None):
    """X under a leading dimension ld (default rows + PAD) with NaN in the padding rows, column-major"""
    X = np.asarray(X, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    ld = X.shape[0] + PAD if ld is None else ld
    out = np.full((ld, X.shape[1]), np.nan, order="F")
    out[:X.shape[0]] = X
    return out


def canary(rows, cols=1):
    return np.full((rows, cols), CANARY, order="F")


def is_canary(X):
    return np.ascontiguousarray(X).view(np.uint64) == CANARY_BITS


def canary_outside(buf, rows, cols):
    """the canary is intact everywhere outside buf[:rows, :cols] and gone everywhere inside"""
    c = is_canary(np.asarray(buf)).reshape(np.asarray(buf).shape)
    inside = np.zeros(c.shape, dtype=bool)
    inside[:rows, :cols] = True
    return bool(np.all(c[~inside])) and not bool(np.any(c[inside]))


# ---- statements ------------------------------------------------------------------------------------------------------------
def _ld_matmul(A, B):
    """A B in extended precision (exact rationals rounded once where the platform has no 64-bit mantissa)"""
    if HAVE_LD:
        return np.asarray(A, dtype=LD) @ np.asarray(B, dtype=LD)
    assert A.shape[1] <= 300, "no extended precision here: only the shapes with at most 300 rows"
    FA = [[Fraction(float(x)) for x in row] for row in np.asarray(A, dtype=np.float64)]
    FB = [[Fraction(float(x)) for x in col] for col in np.asarray(B, dtype=np.float64).T]
    return np.array([[float(sum(a * b for a, b in zip(ra, cb))) for cb in FB] for ra in FA], dtype=LD)


def ld_available(k):
    return HAVE_LD or k <= 300


def int_matmul(A, B):
    A, B = np.asarray(A), np.asarray(B)
    assert np.all(A == np.rint(A)) and np.all(B == np.rint(B))
    out = A.astype(np.int64) @ B.astype(np.int64)
    assert np.abs(A).astype(np.int64).dot(np.abs(B).astype(np.int64)).max(initial=0) < 2 ** 50
    return out


def close(got, want_ld, bound):
    """entrywise |got - want| <= bound, nothing non-finite"""
    got = np.asarray(got)
    return bool(np.all(np.isfinite(got))) and bool(np.all(np.abs(got.astype(LD) - want_ld) <= bound))


def check_product(got, A, B, kind, k, base=None, scale=1.0, extra=0):
    """got == base + scale * A B: exactly (int64) for the exact inputs, within 1.01 (k + extra) 2^-53 (|base| + |A| |B|)
    of the extended-precision statement otherwise (k products per sum; `extra` further roundings of the same magnitude)"""
    if kind == "exact":
        want = int(scale) * int_matmul(A, B) + (0 if base is None else np.asarray(base).astype(np.int64))
        assert np.all(np.isfinite(got)) and np.array_equal(np.asarray(got), want.astype(np.float64)), \
            "exact product differs at %s" % (np.argwhere(np.asarray(got) != want)[:4].tolist(),)
        return 0.0
    want = LD(scale) * _ld_matmul(A, B) + (0 if base is None else np.asarray(base, dtype=LD))
    mag = np.abs(A) @ np.abs(B) + (0 if base is None else np.abs(base))
    bound = 1.01 * (k + extra) * U * mag
    err = np.abs(np.asarray(got).astype(LD) - want)
    assert np.all(np.isfinite(got)) and np.all(err <= bound), "error / bound = %.3g" % float(np.max(err / np.maximum(bound, 1e-300)))
    return float(np.max(err / np.maximum(bound, 1e-300)))


def check_gemm_tn(Cbuf, A, B, p, cb, kind):
    """Cbuf (ldc x ncols, canary-filled before the call) against A[:, :p]' B[:, :cb]; the canary outside p x cb"""
    assert canary_outside(Cbuf, p, cb), "C written outside p x cb, or not everywhere inside"
    return check_product(Cbuf[:p, :cb], A[:, :p].T, B[:, :cb], kind, A.shape[0])


def check_update(Wbuf, mxbuf, Q, C, Ri, W, kind, mx_seed=None):
    """Wbuf (ldw x ncols, the panel followed by canary columns; NaN padding rows) after W <- (W - Q C) Ri; mxbuf: 16 uint64 after the
    call or None.  Bound: 1.01 (p + cb + 2) 2^-53 ((|W| + |Q| |C|) |Ri|)."""
    n, cb = W.shape
    p = Q.shape[1]
    got = Wbuf[:n, :cb]
    assert np.all(np.isnan(Wbuf[n:, :cb])) and np.all(is_canary(Wbuf[:, cb:])), "k_update wrote outside n x cb"
    if kind == "exact":
        want = (W.astype(np.int64) - int_matmul(Q, C)) @ Ri.astype(np.int64) if p else W.astype(np.int64) @ Ri.astype(np.int64)
        assert np.abs(want).max() < 2 ** 50
        assert np.array_equal(got, want.astype(np.float64)), "exact update differs at %s" % (np.argwhere(got != want)[:4].tolist(),)
    else:
        T = np.asarray(W, dtype=LD) - (_ld_matmul(Q, C) if p else 0)
        want = T @ np.asarray(Ri, dtype=LD)
        bound = 1.01 * (p + cb + 2) * U * ((np.abs(W) + (np.abs(Q) @ np.abs(C) if p else 0)) @ np.abs(Ri))
        err = np.abs(got.astype(LD) - want)
        assert np.all(np.isfinite(got)) and np.all(err <= bound), "error / bound = %.3g" % float(np.max(err / bound))
    if mxbuf is not None:
        # bit for bit the column maxima of |W| as it came back from the same call; a larger seed survives; the rest untouched
        want_mx = np.abs(got).max(axis=0)
        if mx_seed is not None:
            want_mx = np.maximum(want_mx, mx_seed[:cb])
        assert np.array_equal(mxbuf[:cb], want_mx.view(np.uint64)), "column maxima differ"
        assert np.all(mxbuf[cb:] == CANARY_BITS), "mx[cb .. 15] touched"


def round_cols_statement(X, slices, mx=None):
    """k_round_cols in numpy, as the kernel does it: per column frexp(ldexp(0.98, 8 S - 1) / m), qs = 2^(e - 1), rint (ties to
    even, like llrint) through int64 (a negative value that rounds to zero comes back as +0, as (double)llrint gives it), times
    2^(1 - e); an all-zero column stays as it is"""
    X = np.array(X, dtype=np.float64, order="F")
    for j in range(X.shape[1]):
        m = np.abs(X[:, j]).max() if mx is None else mx[j]
        if not m > 0:
            continue
        e = int(np.frexp(np.ldexp(0.98, 8 * slices - 1) / m)[1])
        X[:, j] = np.rint(X[:, j] * np.ldexp(1.0, e - 1)).astype(np.int64).astype(np.float64) * np.ldexp(1.0, 1 - e)
    return X


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


def round_matrix(rows, seed):
    """columns for the rounding: normal, all zero, maximum a power of two, entries exactly on rounding ties (odd multiples of
    half a grid step under a power-of-two maximum), all negative, and one small against the others"""
    rng = np.random.default_rng([73, seed, rows])
    X = np.zeros((rows, 6), order="F")
    X[:, 0] = rng.standard_normal(rows)
    X[:, 2] = rng.uniform(-1, 1, rows) * 0.25
    X[rows // 2, 2] = -0.25
    # the ties depend on the grid: callers that round at S slices replace this column by tie_column(rows, S, ...)
    X[:, 3] = tie_column(rows, 1, seed)
    X[:, 4] = -np.abs(rng.standard_normal(rows)) - 0.5
    X[:, 5] = rng.standard_normal(rows) * 2.0 ** -40
    return X


def tie_column(rows, slices, seed):
    """maximum exactly 1, every other entry an odd multiple of half the grid step of k_round_cols at `slices`: all on a tie"""
    e = int(np.frexp(np.ldexp(0.98, 8 * slices - 1))[1])
    step = np.ldexp(1.0, 1 - e)
    rng = np.random.default_rng([74, seed, rows, slices])
    k = rng.integers(-40, 40, size=rows) * 2 + 1
    x = k * (step / 2)
    x[0] = 1.0
    return x


# ---- the tiling of the kernels restated, with named mutants (for the CPU test only) ---------------------------------------------
TN_MUTANTS = ("no_tail", "odd_last_group_skipped", "chunk_ge_4_not_added", "bval_ignored")
UP_MUTANTS = ("one_tile_reuse_above_128", "mx_not_cleared")


def gemm_tn_tiled(A, B, p, cb, ldc, mutant=None):
    """k_gemm_tn<1|2> + k_gemm_tn_reduce: chunks of 1024 rows, four waves of 256 rows each, groups of 32 rows through two
    register sets (the odd last group is multiplied by the first set alone), a tail in steps of 8 rows, the four waves' sums
    added pairwise, then four interleaved running sums over the chunks, added pairwise.  Returns the canary-filled C buffer
    (ldc x 32) as the device would leave it."""
    rows = A.shape[0]
    nt = (cb + 15) // 16
    ncol = 16 * nt
    # columns past cb: read from column 0 and masked to zero by bval
    Bt = np.zeros((rows, ncol))
    Bt[:, :cb] = B[:, :cb]
    if mutant == "bval_ignored":
        Bt[:, cb:] = B[:, [0]]
    nrc = (rows + 1023) // 1024
    partial = np.zeros((nrc, p, ncol))
    for rc in range(nrc):
        c0, c1 = rc * 1024, min(rc * 1024 + 1024, rows)
        wsum = []
        for wave in range(4):
            r0 = c0 + 256 * wave
            r1 = min(r0 + 256, c1)
            acc = np.zeros((p, ncol))
            nfull = (r1 - r0) // 32 if r1 > r0 else 0
            for g in range(0, nfull, 2):
                acc += A[r0 + 32 * g:r0 + 32 * g + 32, :p].T @ Bt[r0 + 32 * g:r0 + 32 * g + 32]
                if g + 1 < nfull:
                    acc += A[r0 + 32 * g + 32:r0 + 32 * g + 64, :p].T @ Bt[r0 + 32 * g + 32:r0 + 32 * g + 64]
            if mutant == "odd_last_group_skipped" and nfull % 2 == 1:
                g = nfull - 1
                acc -= A[r0 + 32 * g:r0 + 32 * g + 32, :p].T @ Bt[r0 + 32 * g:r0 + 32 * g + 32]
            if mutant != "no_tail":
                for r in range(r0 + 32 * nfull, r1, 8):
                    acc += A[r:min(r + 8, r1), :p].T @ Bt[r:min(r + 8, r1)]
            wsum.append(acc)
        partial[rc] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3])
    parts = []
    for part in range(4):
        s = np.zeros((p, ncol))
        for c in range(part, nrc, 4):
            if mutant == "chunk_ge_4_not_added" and c >= 4:
                continue
            s += partial[c]
        parts.append(s)
    total = (parts[0] + parts[1]) + (parts[2] + parts[3])
    C = canary(ldc, 32)
    keep = ncol if mutant == "bval_ignored" else cb    # (the reduce's own column test goes with the mask)
    C[:p, :keep] = total[:, :keep]
    return C


def update_tiled(Q, C, Ri, W, ldw, mx_in=None, mutant=None, stale=1.0e6):
    """k_update<8|16>: a workgroup covers 1024 rows in four turns of 256; the coefficients go through LDS in tiles of 128 basis
    columns, and a single tile (p <= 128) stays there for the turns after the first; the column maxima go through a zeroed LDS
    array and one atomic max per workgroup and column.  Returns (W buffer with NaN padding and two canary columns, mx or None)."""
    n, cb = W.shape
    p = Q.shape[1]
    CBT = 8 if cb <= 8 else 16
    one_tile = p <= 128 or mutant == "one_tile_reuse_above_128"
    out = np.full((ldw, cb + 2), CANARY, order="F")
    out[:, :cb] = np.nan
    mx = None if mx_in is None else np.array(mx_in, dtype=np.uint64)
    for wg in range((n + 1023) // 1024):
        sS = np.zeros((128, CBT))
        smx = np.full(cb, stale if mutant == "mx_not_cleared" else 0.0)
        for it in range(4):
            i0 = (wg * 4 + it) * 256
            i1 = min(i0 + 256, n)
            acc = np.zeros((max(i1 - i0, 0), CBT))
            for a0 in range(0, p, 128):
                ta = min(128, p - a0)
                if not (one_tile and it > 0):
                    sS[:ta] = 0.0
                    sS[:ta, :cb] = C[a0:a0 + ta, :cb]
                if i1 > i0:
                    acc += Q[i0:i1, a0:a0 + ta] @ sS[:ta]
            if i1 > i0:
                res = (W[i0:i1] - acc[:, :cb]) @ Ri
                out[i0:i1, :cb] = res
                smx = np.maximum(smx, np.abs(res).max(axis=0))
        if mx is not None:
            mx[:cb] = np.maximum(mx[:cb], smx.view(np.uint64))
    return out, mx


# ---- the fused step ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused_input(nr, p, cb, deficient=False):
    """(Q, W): Q (nr x p) from a numpy QR, rounded to the 16-bit grid as a solve stores it; W (nr x cb) standard normal, or
    with its last column an exact copy of its first (rank deficient; cb >= 2)"""
    rng = np.random.default_rng([75, nr, p, cb])
    Q = np.zeros((nr, 0), order="F")
    if p:
        Q = round_cols_statement(np.linalg.qr(rng.standard_normal((nr, p)))[0], 2)
    W = np.asfortranarray(rng.standard_normal((nr, cb)))
    if deficient:
        W[:, cb - 1] = W[:, 0]
    Q.setflags(write=False)
    W.setflags(write=False)
    return Q, W


def fused_residuals(Q, W, Wn):
    """max |Wn'Wn - I|, max |Q'Wn|, max |(I - Wn Wn')(I - Q Q') W| / max |W|, in extended precision"""
    Ql, Wl, Wnl = (np.asarray(X, dtype=LD) for X in (Q, W, Wn))
    cb = W.shape[1]
    r1 = float(np.abs(Wnl.T @ Wnl - np.eye(cb, dtype=LD)).max())
    r2 = float(np.abs(Ql.T @ Wnl).max()) if Q.shape[1] else 0.0
    P = Wl - Ql @ (Ql.T @ Wl) if Q.shape[1] else Wl
    r3 = float(np.abs(P - Wnl @ (Wnl.T @ P)).max() / np.abs(Wl).max())
    return r1, r2, r3
