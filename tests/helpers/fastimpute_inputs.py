"""What the tests of snp_fastImpute share (tests/test_fastimpute_cpu.py, tests/test_gpu_fastimpute.py): a direct numpy
definition of the statement of bigsnpr_amd/csrc/fastimpute_step.hpp (Philox, exp_det and log_det ported line by line; a
recursive tree, not the level-wise walk of the kernels and the CPU statement), the masked example.bed case of the
reference's own test with predictor lists from a numpy correlation, seeded synthetic images, and the constants of
fastimpute.hip read from its source."""
import math
import os
import re
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

import fastimpute_ref as ref  # noqa: E402
from impute_ref import read_bed_bytes  # noqa: E402

FAST_HIP = os.path.join(ROOT, "bigsnpr_amd", "csrc", "fastimpute.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")
TAG = 0x46494D50   # "FIMP"
SEED = 20261020    # chosen before any result was looked at; tests/test_fastimpute_cpu.py says what it gives
Q = 2.0 ** 30


# ---- the generator and the two functions, ported ----------------------------------------------------------------------------
def philox4x32_10(c, k):
    c = [np.asarray(x, dtype=np.uint64) for x in c]
    k0, k1 = int(k[0]), int(k[1])
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        a, b = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(b >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), b & M, (a >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), a & M]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def unit_open(a, b):
    n = (a << np.uint64(20)) | (b >> np.uint64(12))
    return (2.0 * n.astype(np.float64) + 1.0) * 2.0 ** -53


LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
EXP_DEN = (6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0)


def exp_det(x):
    """gibbs_step.hpp's exp_det, operation for operation"""
    if x < -708.0:
        return 0.0
    if x > 709.0:
        return math.inf
    k = int(x * 1.4426950408889634 + (-0.5 if x < 0 else 0.5))   # int() truncates like the C cast
    r = (x - k * LN2_HI) - k * LN2_LO
    s = 1.0 / EXP_DEN[0]
    for d in EXP_DEN[1:]:
        s = s * r + 1.0 / d
    s = s * r + 0.5
    s = s * r + 1.0
    s = s * r + 1.0
    k1 = int(k / 2)            # C's k / 2 truncates toward zero
    k2 = k - k1
    return s * math.ldexp(1.0, k1) * math.ldexp(1.0, k2)


def log_det(x):
    """gibbs_step.hpp's log_det, operation for operation"""
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    e = (b >> 52) - 1023
    m = struct.unpack("<d", struct.pack("<Q", (b & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000))[0]
    if m > 1.4142135623730951:
        m = m * 0.5
        e = e + 1
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    t = 1.0 / 23.0
    for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        t = t * z + 1.0 / d
    t = t * z + 1.0
    return e * LN2_HI + (2.0 * s * t + e * LN2_LO)


def prob(margin):
    return 1.0 / (1.0 + exp_det(-margin))


# ---- the statement, directly ----------------------------------------------------------------------------------------------------
def _real(s):
    return float(int(s)) * 2.0 ** -30


def _gain(G, H):
    g = _real(G)
    return g * g / (_real(H) + 1.0)


def numpy_target(G, j, P, p_train, seed):
    """one target of the statement on FBM bytes G (n x m, > 2 = missing): (column of bytes afterwards, infos[1], trees),
    trees = per round the list of (depth, feature position, t, direction) of its splits in preorder"""
    G = np.asarray(G, dtype=np.uint8)
    n = G.shape[0]
    col = G[:, j]
    obs = col <= 2
    i = np.arange(n, dtype=np.uint64)
    z = np.zeros(n, dtype=np.uint64)
    o = philox4x32_10([i, z + np.uint64(j), z + np.uint64(TAG), z], (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    train = obs & (unit_open(o[0], o[1]) < p_train)
    if not train.any():
        train = obs.copy()
    valid = obs & ~train
    y = np.where(obs, col, 0) * 0.5
    T, c1, c2 = int(train.sum()), int((col[train] == 1).sum()), int((col[train] == 2).sum())
    base = min(max((0.5 * c1 + c2) / T, 1e-7), 1.0 - 1e-7)
    margin = np.full(n, log_det(base) - log_det(1.0 - base))
    X = np.minimum(G[:, np.asarray(P, dtype=np.int64)], 3).astype(np.int64).reshape(n, len(P))
    trees = []
    for _ in range(10):
        p = np.array([prob(v) for v in margin])
        gq = np.rint((p - y) * Q).astype(np.int64)
        hq = np.maximum(1, np.rint(np.maximum(p * (1.0 - p), 1e-16) * Q).astype(np.int64))
        add = np.zeros(n)
        splits = []

        def grow(members, depth):
            tr = members & train
            Gs, Hs = int(gq[tr].sum()), int(hq[tr].sum())
            best, best_chg = None, 1e-6
            if depth < 4:
                for f in range(X.shape[1]):
                    for t in (0, 1, 2):
                        for d in (0, 1):
                            left = np.where(X[:, f] == 3, d == 1, X[:, f] < t + 0.5)
                            GL, HL = int(gq[tr & left].sum()), int(hq[tr & left].sum())
                            GR, HR = Gs - GL, Hs - HL
                            if not (_real(HL) >= 1.0 and _real(HR) >= 1.0):
                                continue
                            chg = (_gain(GL, HL) + _gain(GR, HR)) - _gain(Gs, Hs)
                            if chg > best_chg:
                                best, best_chg = (f, t, d, left), chg
            if best is None:
                add[members] = 0.3 * (-_real(Gs) / (_real(Hs) + 1.0))
                return
            splits.append((depth, best[0], best[1], best[2]))
            grow(members & best[3], depth + 1)
            grow(members & ~best[3], depth + 1)

        grow(np.ones(n, dtype=bool), 0)
        margin = margin + add
        trees.append(splits)
    call = np.array([int(np.rint(2.0 * prob(v))) for v in margin], dtype=np.int64)
    out = col.copy()
    out[~obs] = 4 + call[~obs]
    err = float((call[valid] != col[valid]).sum()) / float(valid.sum()) if valid.any() else math.nan
    return out, err, trees


def numpy_fast_impute(G, preds, p_train, seed):
    """every variant of the statement: (bytes, infos 2 x m, n_all_missing); preds = a list of m index sequences"""
    G = np.asarray(G, dtype=np.uint8)
    n, m = G.shape
    out = np.where(G > 2, 3, G).astype(np.uint8)
    infos = np.full((2, m), np.nan)
    n_all = 0
    for j in range(m):
        miss = int((G[:, j] > 2).sum())
        infos[0, j] = miss / n
        n_all += miss == n
        if 0 < miss < n:
            out[:, j], infos[1, j], _ = numpy_target(G, j, preds[j], p_train, seed)
    return out, infos, n_all


def trace_splits(tr):
    """the first-round tree of the CPU statement's trace (31 x 3: feature, t, direction; -1 leaf, -2 absent) as the preorder
    list of (depth, feature, t, direction) that numpy_target gives"""
    out = []

    def walk(k, depth):
        if k < 31 and tr[k, 0] >= 0:
            out.append((depth, int(tr[k, 0]), int(tr[k, 1]), int(tr[k, 2])))
            walk(2 * k + 1, depth + 1)
            walk(2 * k + 2, depth + 1)

    walk(0, 0)
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def random_image(n, m, seed, missing=0.1, ld=True):
    """seeded calls with `missing` of them gone; with ld, neighbouring variants are noisy copies of each other, so that
    trees find something to split on"""
    rng = np.random.default_rng(seed)
    g = np.empty((n, m), dtype=np.uint8)
    g[:, 0] = rng.integers(0, 3, n)
    for j in range(1, m):
        keep = rng.random(n) < (0.8 if ld else 0.0)
        g[:, j] = np.where(keep, g[:, j - 1], rng.integers(0, 3, n))
    g[rng.random((n, m)) < missing] = 3
    return np.asfortranarray(g)


def window_lists(m, width, exclude_self=True):
    """the `width` nearest variants on either side of each variant"""
    return [np.array([k for k in range(max(0, j - width), min(m, j + width + 1)) if k != j], dtype=np.int32) for j in range(m)]


def example_case():
    """test-3-fastImpute.R:21-40 on tests/golden/example.bed (517 x 4542, complete): the variants whose largest correlation
    with another variant within 500 positions exceeds 0.6 get 100 calls masked each (seeded).  Returns a dict: G0 (the
    complete bytes), G (masked), ind (those variants), chr (the chromosome of every variant)."""
    n, m = 517, 4542
    G0 = read_bed_bytes(os.path.join(GOLDEN, "example.bed"), n, m)
    with open(os.path.join(GOLDEN, "example.bim")) as f:
        chrom = np.array([int(line.split()[0]) for line in f])
    assert chrom.size == m and not (G0 == 3).any()
    X = G0.astype(np.float64)
    X -= X.mean(0)
    sd = np.sqrt((X * X).sum(0))
    best = np.full(m, -np.inf)
    for j0 in range(0, m, 512):     # blocks of targets against their window of 500 on either side
        j1 = min(m, j0 + 512)
        lo, hi = max(0, j0 - 500), min(m, j1 + 500)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = (X[:, lo:hi].T @ X[:, j0:j1]) / np.outer(sd[lo:hi], sd[j0:j1])
        k, j = np.meshgrid(np.arange(lo, hi), np.arange(j0, j1), indexing="ij")
        r[(np.abs(k - j) > 500) | (k == j) | ~(r < 1)] = -np.inf
        best[j0:j1] = r.max(0)
    ind = np.flatnonzero(best > 0.6)
    rng = np.random.default_rng(SEED)
    G = G0.copy()
    for j in ind:
        G[rng.choice(n, 100, replace=False), j] = 3
    return dict(G0=G0, G=np.asfortranarray(G), ind=ind, chr=chrom, n=n, m=m)


def numpy_lists(G, chrom, targets, alpha=1e-4, size=200):
    """the predictor lists snp_fastImpute builds, from a numpy correlation on the pairwise complete samples (R/corr.R:
    |r| above the threshold of `alpha` for the number of complete pairs), for `targets` only; the others get none"""
    from bigsnpr_amd.ld import _cor_thresholds
    from bigsnpr_amd.impute import MIN_PREDICTORS
    n, m = G.shape
    thr = _cor_thresholds(n, alpha, 0.0, n_min=3)
    preds = [np.zeros(0, dtype=np.int32)] * m
    for j in targets:
        same = np.flatnonzero(chrom == chrom[j])
        near = same[(np.abs(same - j) <= size) & (same != j)]
        got = []
        for k in near:
            ok = (G[:, j] <= 2) & (G[:, k] <= 2)
            nona = int(ok.sum())
            if nona < 3:
                continue
            x, y = G[ok, j].astype(np.float64), G[ok, k].astype(np.float64)
            x, y = x - x.mean(), y - y.mean()
            den = math.sqrt((x * x).sum() * (y * y).sum())
            if den > 0 and abs((x * y).sum() / den) > thr[nona - 1]:
                got.append(k)
        preds[j] = np.array(got if len(got) >= MIN_PREDICTORS else near, dtype=np.int32)
    return preds


def f_test_through_origin(y, x):
    """anova(lm(y ~ x - 1)): (F, p, slope) with 1 and len(y) - 1 degrees of freedom"""
    from scipy import stats
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    slope = (x * y).sum() / (x * x).sum()
    rss = ((y - slope * x) ** 2).sum()
    F = (slope * slope * (x * x).sum()) / (rss / (y.size - 1))
    return F, float(stats.f.sf(F, 1, y.size - 1)), slope


# ---- the constants of the kernels, from the source ----------------------------------------------------------------------------
def kernel_constants():
    with open(FAST_HIP) as f:
        text = f.read()
    out = {}
    for name in ("kBoostThreads", "kFeatTurn", "kGridTargets", "kLdsSamples"):
        found = re.findall(r"^\s*constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text, flags=re.M)
        assert len(found) == 1, name
        out[name] = int(found[0])
    assert re.search(r"^\s*constexpr\s+int64_t\s+kTurnSamples\s*=\s*4\s*\*\s*kBoostThreads\s*;", text, flags=re.M)
    out["kTurnSamples"] = 4 * out["kBoostThreads"]
    return out
