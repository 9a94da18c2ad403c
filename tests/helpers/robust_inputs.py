"""Inputs and references of tests/test_gpu_robust_kernels.py (the kernels of bigsnpr_amd/csrc/robust.hip), plain numpy, seeded,
no GPU.  tests/test_robust_inputs_cpu.py shows without a GPU that these inputs have teeth.

* key generators: doubles whose order-preserving 64-bit images force every one of the eight byte passes of the radix select
  (k_sel_hist + k_sel_pick) to choose between occupied bins and to carry a non-trivial rank into the next pass;
* exact_median / exact_mad: selection on a sort, the definition the device medians are compared with bit for bit;
* select_emulated: the eight passes restated, with named mutants — only for the CPU test, no GPU test calls it;
* np.longdouble restatements of the definitions in the kernels' comments (scaleTau2, rolling mean, the plain products, the
  medcouple's counts and windows), and the host loop of dist_ogk put together from them.
Nothing here calls bigsnpr_amd.autosvd."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)          # 2^-52
SIGN = np.uint64(1) << np.uint64(63)
Q75 = 0.674489750196081743                       # qnorm(3/4)


# ---- keys -----------------------------------------------------------------------------------------------------------------------
def _from_bits(b):
    x = np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)
    assert np.all(np.isfinite(x))
    return x


def low_bytes(m, base=1.5, negate=False, seed=0):
    """bit pattern of `base` plus a uniform integer in [0, 2^32): the upper four bytes of all keys are equal, the lower four
    decide (`base` has zero low bytes, so nothing carries upwards)"""
    b0 = np.array([base], dtype=np.float64).view(np.uint64)[0]
    assert b0 & np.uint64(0xFFFFFFFF) == 0
    rng = np.random.default_rng([11, seed, m])
    x = _from_bits(b0 + rng.integers(0, 1 << 32, size=m, dtype=np.uint64))
    return -x if negate else x


EVERY_TOP = np.array([0x3F, 0x40, 0xBF, 0xC0], dtype=np.uint64)
EVERY_LOW = np.array([0x11, 0x5A, 0xA3, 0xEC], dtype=np.uint64)


def every_pass(m, seed=0):
    """top byte from four values (two per sign), each of the seven lower bytes from four well-separated values: the bucket of
    the median shrinks by four per pass, so that at m = 40 000 it holds about 10 000, 2 500, 625, 156, 39, 10, 2, 1 keys"""
    rng = np.random.default_rng([12, seed, m])
    b = EVERY_TOP[rng.integers(0, 4, size=m)] << np.uint64(56)
    for shift in range(48, -8, -8):
        b |= EVERY_LOW[rng.integers(0, 4, size=m)] << np.uint64(shift)
    return _from_bits(b)


def one_byte(m, base=-2.75, seed=0):
    """only the lowest byte varies: at most 256 distinct keys, heavy ties in the last pass"""
    b0 = np.array([base], dtype=np.float64).view(np.uint64)[0]
    rng = np.random.default_rng([13, seed, m])
    return _from_bits(b0 | rng.integers(0, 256, size=m, dtype=np.uint64))


def around_zero(m, seed=0):
    """signed denormals k 2^-1074, |k| <= 6, with both zeros"""
    rng = np.random.default_rng([14, seed, m])
    k = rng.integers(-6, 7, size=m)
    x = k.astype(np.float64) * 2.0 ** -1074
    x[(k == 0) & (rng.random(m) < 0.5)] = -0.0
    return x


GENERATORS = (
    lambda m, s: low_bytes(m, 1.5, False, s),
    lambda m, s: every_pass(m, s),
    lambda m, s: low_bytes(m, 1.5, True, s),
    lambda m, s: one_byte(m, -2.75, s),
    lambda m, s: around_zero(m, s),
    lambda m, s: low_bytes(m, 2.0 ** -300, bool(s & 1), s),
    lambda m, s: one_byte(m, 3.0e5, s),
)
GENERATOR_NAMES = ("low_bytes", "every_pass", "low_bytes negated", "one_byte", "around_zero", "low_bytes tiny", "one_byte large")
MEDIAN_M = (1, 2, 3, 255, 256, 257, 16384, 16385, 40000, 40001)
MEDIAN_NCOL = (1, 7, 33)
PAD = 37                                         # ld = m + PAD in the padded cases


def median_matrix(m, ncol):
    """m x ncol, column c from generator c mod 7 with a seed of its own: the first columns of a wider matrix are the narrower
    matrix, and no two columns are equal"""
    return np.column_stack([GENERATORS[c % len(GENERATORS)](m, c) for c in range(ncol)])


def exact_median(x):
    s = np.sort(np.asarray(x, dtype=np.float64))
    m = s.size
    return 0.5 * (s[(m - 1) // 2] + s[m // 2])


def exact_mad(x, c):
    return exact_median(np.abs(np.asarray(x, dtype=np.float64) - c))


def exact_medians(X, centre=None):
    """column by column (axis 0 of an m x ncol matrix)"""
    X = np.asarray(X, dtype=np.float64)
    if centre is not None:
        X = np.abs(X - np.asarray(centre)[None, :])
    s = np.sort(X, axis=0)
    m = s.shape[0]
    return 0.5 * (s[(m - 1) // 2] + s[m // 2])


def padded(X, ld, fill=np.nan):
    """flat column-major buffer with ld - m rows of `fill` under every column: a kernel that reads a padding row poisons its
    result"""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    buf = np.full((ld, X.shape[1]), fill, dtype=np.float64, order="F")
    buf[: X.shape[0]] = X
    return buf.ravel(order="F")


def unpadded(buf, m, ld, ncol):
    """(the m x ncol matrix, the padding rows) of such a buffer"""
    a = np.asarray(buf).reshape((ld, ncol), order="F")
    return a[:m], a[m:]


# ---- the radix select, restated ---------------------------------------------------------------------------------------------------
PASS_MUTANTS = tuple("skip%d" % s for s in range(56, -8, -8)) + ("rank_kept_low", "no_complement")
RANK_MUTANTS = ("both_upper", "both_lower")
MUTANTS = PASS_MUTANTS + RANK_MUTANTS
# (m - 1) / 2 and m / 2 exchanged between the two virtual columns: the median is 0.5 (a + b) either way, the same bits on every
# input — an equivalent program, not a mutant that any test could catch (test_robust_inputs_cpu.py asserts the identity)
EQUIVALENT = ("ranks_swapped",)


def keys_of(x, mutant=None):
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    if mutant == "no_complement":                # negative values keep their magnitude bits: they sort backwards
        return b ^ SIGN
    return np.where(b >> np.uint64(63) != 0, ~b, b | SIGN)


def value_of(k, mutant=None):
    k = np.uint64(k)
    if mutant == "no_complement":
        b = k ^ SIGN
    else:
        b = (k & ~SIGN) if (k >> np.uint64(63)) else ~k
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def select_emulated(x, rank, mutant=None, trace=None):
    """order statistic `rank` (0-based) of x as k_sel_hist + k_sel_pick find it: eight passes over the bytes of the keys, high
    to low.  trace: a list that receives, per pass, (keys that match the prefix, keys in the chosen bin, occupied bins,
    keys below the chosen bin)."""
    assert mutant is None or mutant in PASS_MUTANTS
    k = keys_of(x, mutant)
    prefix, r = np.uint64(0), int(rank)
    for shift in range(56, -8, -8):
        himask = np.uint64(0) if shift >= 56 else np.uint64((~0 << (shift + 8)) & 0xFFFFFFFFFFFFFFFF)
        match = (k & himask) == (prefix & himask)
        hist = np.bincount(((k[match] >> np.uint64(shift)) & np.uint64(255)).astype(np.int64), minlength=256)
        if mutant == "skip%d" % shift:
            continue
        cum = np.cumsum(hist)
        over = np.nonzero(cum > r)[0]
        b, below = (int(over[0]), int(cum[over[0]] - hist[over[0]])) if over.size else (255, int(cum[-1]))
        if trace is not None:
            trace.append((int(match.sum()), int(hist[b]), int((hist > 0).sum()), below))
        if not (mutant == "rank_kept_low" and shift <= 24):
            r -= below
        prefix |= np.uint64(b) << np.uint64(shift)
    return value_of(prefix, mutant)


def median_emulated(x, mutant=None):
    m = np.asarray(x).size
    lo, hi = (m - 1) // 2, m // 2
    if mutant == "both_upper":
        lo = hi
    elif mutant == "both_lower":
        hi = lo
    elif mutant == "ranks_swapped":
        lo, hi = hi, lo
    pm = mutant if mutant in PASS_MUTANTS else None
    a = select_emulated(x, lo, pm)
    b = a if hi == lo else select_emulated(x, hi, pm)
    return 0.5 * (a + b)


# ---- scaleTau2 ------------------------------------------------------------------------------------------------------------------
def erho_of(b):
    """Erho(b) of robustbase::scaleTau2 (consistency = TRUE)"""
    Phi, phi = 0.5 * math.erfc(-b / math.sqrt(2.0)), math.exp(-0.5 * b * b) / math.sqrt(2.0 * math.pi)
    return 2.0 * ((1.0 - b * b) * Phi - b * phi + b * b) - 1.0


def _tau2_rows(rows, k, m, c1, c2):
    """scaleTau2 of k vectors of length m; rows(c0, c1) returns vectors c0 ... c1 - 1 as the rows of a contiguous matrix"""
    mu, s = np.empty(k), np.empty(k)
    erho = LD(erho_of(c2 * Q75))
    step = max(1, (1 << 19) // m)
    lo, hi = (m - 1) // 2, m // 2

    def chunk(c0):
        A = rows(c0, min(k, c0 + step))
        S = np.sort(A, axis=1)
        med = 0.5 * (S[:, lo] + S[:, hi])
        S = np.sort(np.abs(A - med[:, None]), axis=1)
        mad = 0.5 * (S[:, lo] + S[:, hi])
        ok = mad > 0
        s0 = np.where(ok, mad, 1.0).astype(LD)[:, None]
        AL, medL = A.astype(LD), med.astype(LD)[:, None]
        t = np.abs(AL - medL) / (s0 * LD(c1))
        w = np.maximum(LD(0), LD(1) - t * t)
        w = w * w
        muL = (AL * w).sum(axis=1) / w.sum(axis=1)
        t = (AL - muL[:, None]) / s0
        rho = np.minimum(t * t, LD(c2) * LD(c2))
        sL = s0[:, 0] * np.sqrt(rho.sum(axis=1) / (LD(m) * erho))
        mu[c0:c0 + step] = np.where(ok, muL.astype(np.float64), med)
        s[c0:c0 + step] = np.where(ok, sL.astype(np.float64), 0.0)

    starts = range(0, k, step)
    if len(starts) > 2:                          # numpy's loops release the interpreter lock: same values, any order
        with ThreadPoolExecutor(max_workers=min(8, len(starts))) as ex:
            list(ex.map(chunk, starts))
    else:
        for c0 in starts:
            chunk(c0)
    return mu, s


def tau2_ref_cols(X, c1=4.5, c2=3.0):
    """robustbase::scaleTau2(mu.too = TRUE) of every column of the m x k matrix X -> (mu [k], s [k]), float64.  The median and
    the MAD are exact selections on a sort of the float64 values (what bsn_robust_medians is pinned to, bit for bit); the
    weighted mean and the truncated second moment are sums in np.longdouble.  (median, 0) where the MAD is 0."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    return _tau2_rows(lambda c0, c1_: np.ascontiguousarray(X[:, c0:c1_].T), X.shape[1], X.shape[0], c1, c2)


def tau2_ref(x, c1=4.5, c2=3.0):
    mu, s = tau2_ref_cols(np.asarray(x, dtype=np.float64)[:, None], c1, c2)
    return float(mu[0]), float(s[0])


TAU2_CONSTANTS = ((4.5, 3.0), (3.0, 2.0), (6.0, 1.5))
TAU2_MAD0, TAU2_CONST = 5, 6                      # columns of tau2_matrix with MAD 0 / constant


def tau2_matrix(m, ncol=33):
    """ordinary columns (Student t, their own locations and scales, a block of outliers) with a MAD-0 column (7 in 10 values
    equal) and a constant column between them"""
    rng = np.random.default_rng([21, m])
    X = rng.standard_t(3, size=(m, ncol)) * rng.uniform(0.2, 30.0, size=ncol) + rng.normal(size=ncol) * 5.0
    X[: m // 40] += 50.0
    X[:, TAU2_MAD0] = np.where(rng.random(m) < 0.7, 0.5, X[:, TAU2_MAD0])
    X[:, TAU2_CONST] = -3.25
    if m == 2:
        X[1, TAU2_MAD0] = X[0, TAU2_MAD0]
    return X


def pair_list(p):
    """the documented order of bsn_robust_pair_scales: (1,0), (2,0), (2,1), (3,0) ..."""
    return [(i, j) for i in range(p) for j in range(i)]


def pair_matrix(m, p=64):
    """columns on the scale the OGK loop hands over (about 1), correlated, with a block of outlying rows"""
    rng = np.random.default_rng([22, m, p])
    Z = rng.normal(size=(m, p))
    Z += 0.6 * rng.normal(size=(m, 1)) * rng.uniform(-1, 1, size=p)
    Z *= rng.uniform(0.7, 1.4, size=p)
    Z[: max(1, m // 50)] += 3.0
    return Z


def pair_scales_ref(Z, pairs, c1=4.5, c2=3.0):
    """scaleTau2 of Z_i + Z_j and of Z_i - Z_j (the float64 sums and differences) for the given pairs"""
    i, j = np.array([q[0] for q in pairs]), np.array([q[1] for q in pairs])
    Zt = np.ascontiguousarray(np.asarray(Z, dtype=np.float64).T)
    m = Zt.shape[1]
    return (_tau2_rows(lambda a, b: Zt[i[a:b]] + Zt[j[a:b]], len(pairs), m, c1, c2)[1],
            _tau2_rows(lambda a, b: Zt[i[a:b]] - Zt[j[a:b]], len(pairs), m, c1, c2)[1])


# ---- plain products ---------------------------------------------------------------------------------------------------------------
def rotate_ref(Z, E):
    """Z E in np.longdouble, and |Z| |E| (the sum of absolute terms behind every entry)"""
    ZL, EL = np.asarray(Z).astype(LD), np.asarray(E).astype(LD)
    return ZL @ EL, (np.abs(ZL) @ np.abs(EL)).astype(np.float64)


def wdist_ref(Z, mu, sig):
    t = (np.asarray(Z).astype(LD) - np.asarray(mu).astype(LD)) / np.asarray(sig).astype(LD)
    return (t * t).sum(axis=1)


def mahalanobis_ref(U, centre, P):
    X = np.asarray(U).astype(LD) - np.asarray(centre).astype(LD)
    return ((X @ np.asarray(P).astype(LD)) * X).sum(axis=1)


def product_matrix(m, p):
    rng = np.random.default_rng([23, m, p])
    return rng.normal(size=(m, p)) * rng.uniform(0.5, 2.0, size=p) + rng.normal(size=p)


# ---- dist_ogk ---------------------------------------------------------------------------------------------------------------------
OGK_M = 4097
OGK_P = (1, 33, 64)
OGK_NITER = (0, 1, 2)


def ogk_input(p, m=OGK_M):
    """loadings-like columns: scales 0.5 ... 2 mixed by a rotation (a correlation matrix with a spread spectrum, no nearly equal
    eigenvalues), and a block of outlying rows (a long-range LD region)"""
    rng = np.random.default_rng([24, m, p])
    Q = np.linalg.qr(rng.normal(size=(p, p)))[0]
    U = (rng.normal(size=(m, p)) * np.geomspace(0.5, 2.0, p)) @ Q.T
    U[: m // 50] += 4.0 * Q[:, 0]
    return np.ascontiguousarray(U)


def dist_ogk_ref(U, cut_ratio, niters=OGK_NITER, c1=4.5, c2=3.0):
    """bigutilsr::dist_ogk as csrc/robust.hip: dist_ogk states it, from the pieces above: `it` rounds of (scale the columns by
    their tau scales, correlation matrix from the pair scales, rotate by its eigenvectors), then location and scale of the
    rotated columns, wdist, hard rejection at median(wdist) * cut_ratio, centre and covariance (denominator n_kept - 1) of the
    kept rows of U, distances with the pseudo-inverse.  One pass serves every number of rounds in `niters`:
    {niter: dict(dist, n_kept, margin)}, margin = min |wdist / d0 - 1|."""
    U = np.asarray(U, dtype=np.float64)
    m, p = U.shape
    pairs = pair_list(p)
    Z, out = U.copy(), {}
    for it in range(max(niters) + 1):
        if it in niters:
            mu, sig = tau2_ref_cols(Z, c1, c2)
            sig[~(sig > 0)] = 1.0
            wd = wdist_ref(Z, mu, sig).astype(np.float64)
            d0 = exact_median(wd) * cut_ratio
            keep = wd <= d0
            K = U[keep].astype(LD)
            nk = K.shape[0]
            centre = K.sum(axis=0) / LD(nk)
            Kc = K - centre
            cov = ((Kc.T @ Kc) / LD(nk - 1)).astype(np.float64)
            centre = centre.astype(np.float64)
            P = np.linalg.pinv(cov, rcond=1e-15, hermitian=True)
            out[it] = dict(dist=mahalanobis_ref(U, centre, P).astype(np.float64), n_kept=int(nk),
                           margin=float(np.abs(wd / d0 - 1.0).min()))
        if it == max(niters):
            break
        d = tau2_ref_cols(Z, c1, c2)[1]
        d[~(d > 0)] = 1.0
        Z = Z / d
        R = np.eye(p)
        if pairs:
            ss, sd = pair_scales_ref(Z, pairs, c1, c2)
            for t, (i, j) in enumerate(pairs):
                R[i, j] = R[j, i] = (ss[t] * ss[t] - sd[t] * sd[t]) / 4
        E = np.linalg.eigh(R)[1][:, ::-1]
        Z = rotate_ref(Z, E)[0].astype(np.float64)
    return out


def one_ulp_noise(U, seed=0):
    """every entry changed by one relative 2^-52 of random sign"""
    rng = np.random.default_rng([25, seed])
    return U * (1.0 + EPS64 * rng.choice([-1.0, 1.0], size=U.shape))


# ---- medcouple --------------------------------------------------------------------------------------------------------------------
MC_TURN = 262144                                  # 1024 workgroups x 256 threads: the second turn of the grid-stride loop starts here
MC_NU, MC_NL = MC_TURN + 300, 700
MC_T = (-0.9, -0.3, 0.0, 0.4, 0.95)
MC_WINDOWS = {"lognormal": ((-0.2, -0.199), (0.0, 0.001), (0.3, 0.3005), (-0.9, -0.8995), (0.95, 0.9502)),
              "dyadic": ((-1.0 / 512, 0.0), (0.0, 1.0 / 512), (-0.25, -0.2495))}


def mc_input(kind):
    """(up [262 444], lo [700] ascending), positive distances to a median.  `up` is not sorted (the kernels search `lo` only);
    its last 300 values are on the small side, so that some of them count at every t and fall into every window.  kind "dyadic": all values k / 64 — at t = 0 every threshold
    is a value of `lo` or lies between two of them exactly, the side = "left" edge; `lo` has ties."""
    rng = np.random.default_rng([26, int(kind == "dyadic")])
    if kind == "dyadic":
        up = rng.integers(1, 4097, size=MC_NU).astype(np.float64) / 64.0
        up[MC_TURN:] = rng.integers(1, 1025, size=MC_NU - MC_TURN) / 64.0
        lo = np.sort(rng.integers(1, 4097, size=MC_NL)).astype(np.float64) / 64.0
        lo[:40] = np.sort(rng.integers(1, 9, size=40)) / 64.0           # ties, and partners of the small values of `up`
        return up, np.sort(lo)
    up = rng.lognormal(size=MC_NU)
    up[MC_TURN:] = rng.uniform(0.05, 0.5, size=MC_NU - MC_TURN)
    lo = np.sort(np.exp(rng.uniform(np.log(0.002), np.log(40.0), size=MC_NL)))
    return up, lo


def _mc_first(lo, u, t):
    """first index of the ascending lo with lo >= (u (1 - t)) / (1 + t), the threshold in float64 as the kernel and the host
    path compute it: the same integers"""
    return np.searchsorted(lo, (u * (1.0 - t)) / (1.0 + t), side="left")


def mc_count_ref(up, lo, t, first=0):
    """number of pairs (u, l) with (u - l) / (u + l) <= t; first: only up[first:]"""
    return int(np.sum(lo.size - _mc_first(lo, up[first:], t)))


def mc_window_ref(up, lo, a, b, first=0):
    """the kernel values (u - l) / (u + l) in (a, b], ascending"""
    u = up[first:]
    x0 = _mc_first(lo, u, b)
    cnt = np.maximum(_mc_first(lo, u, a) - x0, 0)
    tot = int(cnt.sum())
    ur = np.repeat(u, cnt)
    l = lo[np.repeat(x0 - (np.cumsum(cnt) - cnt), cnt) + np.arange(tot)]
    return np.sort((ur - l) / (ur + l))


# ---- rolling mean -----------------------------------------------------------------------------------------------------------------
def rollmean_weights(length):
    """positive, symmetric, bell-shaped"""
    return np.exp(-0.5 * np.linspace(-2.5, 2.5, length) ** 2) if length > 1 else np.array([0.7])


def rollmean_ref(x, w, offsets=None):
    """out[i] = sum_j w[j] x[i - half + j] / sum_j w[j] over the taps inside the group of i (groups: [offsets[g],
    offsets[g + 1])), in np.longdouble"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    m, half = x.size, w.size // 2
    off = np.array([0, m]) if offsets is None else np.asarray(offsets)
    i = np.arange(m)
    g = np.searchsorted(off, i, side="right") - 1
    lo, hi = off[g], off[g + 1]
    xL, num, den = x.astype(LD), np.zeros(m, dtype=LD), np.zeros(m, dtype=LD)
    for j in range(w.size):
        k = i - half + j
        ok = (k >= lo) & (k < hi)
        num[ok] += LD(w[j]) * xL[k[ok]]
        den[ok] += LD(w[j])
    return num / den


ROLL_CASES = (                                    # (m, taps, group offsets or None)
    (9000, 4095, (0, 300, 301, 4397, 9000)),      # groups of 300, 1, 4096, 4603: two shorter than the window, one of size 1
    (1000, 1, (0, 255, 256, 257, 1000)),
    (1000, 101, (0, 255, 256, 257, 1000)),        # group edges below, on and above a workgroup edge
    (1000, 101, None),
)


def roll_input(m):
    return np.random.default_rng([27, m]).lognormal(size=m)
