"""Shared by test_king_cpu.py and test_gpu_king.py: .bed payloads to and from decoded codes in NumPy, the fixed-seed shapes,
the NumPy restatement of the KING-robust definition and the comparison of two tables.  Not a test module."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
COUNT_NAMES = ("NSNP", "HETHET", "IBS0", "HET1HOM2", "HET2HOM1")
FROM_PLINK = np.array([2, 3, 1, 0], dtype=np.int8)    # .bed bit pairs 00, 01, 10, 11 -> allele count, 3 = missing
TO_PLINK = np.array([3, 2, 0, 1], dtype=np.uint8)


def decode_payload(payload, n, m):
    """n x m codes (0, 1, 2; 3 = missing) of a .bed payload (variant-major, four samples per byte)"""
    b = np.asarray(payload, dtype=np.uint8).reshape(m, (n + 3) // 4)
    f = (b[:, :, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3
    return np.ascontiguousarray(FROM_PLINK[f.reshape(m, -1)[:, :n]].T)


def encode_payload(G):
    n, m = G.shape
    f = np.zeros((m, (n + 3) // 4 * 4), dtype=np.uint8)       # pad samples: bit pair 00, as PLINK writes them
    f[:, :n] = TO_PLINK[np.asarray(G).T]
    f = f.reshape(m, -1, 4)
    return np.ascontiguousarray((f[:, :, 0] | (f[:, :, 1] << 2) | (f[:, :, 2] << 4) | (f[:, :, 3] << 6)).astype(np.uint8)).ravel()


def read_golden(name):
    """(codes n x m, payload, n, m) of tests/golden/<name>.bed"""
    path = os.path.join(GOLDEN, name + ".bed")
    n = sum(1 for _ in open(path[:-4] + ".fam"))
    m = sum(1 for _ in open(path[:-4] + ".bim"))
    raw = np.fromfile(path, dtype=np.uint8)
    assert raw[0] == 0x6C and raw[1] == 0x1B and raw[2] == 1
    payload = raw[3:3 + m * ((n + 3) // 4)]
    return decode_payload(payload, n, m), payload, n, m


def related_example():
    """example.bed as the reference's test prepares it (tests/testthat/test-3-plink-QC.R:90-100): sample 0 becomes
    round((sample 1 + sample 2) / 2), half to even"""
    G, _, n, m = read_golden("example")
    G = G.copy()
    G[0] = np.rint((G[1].astype(np.float64) + G[2]) / 2).astype(np.int8)
    return G


def random_codes(n, m, na, seed):
    """n x m codes from a fixed seed: allele frequencies 0.05 .. 0.5 per variant, a share `na` missing"""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.5, size=m)
    G = rng.binomial(2, af, size=(n, m)).astype(np.int8)
    if na > 0:
        G[rng.random((n, m)) < na] = 3
    return G


def numpy_table(G):
    """the definition through the plane products, in NumPy: int64 matrix products, then the double in the order of
    king_step.hpp (one division, one subtraction)"""
    G = np.asarray(G).astype(np.int64)
    P = (G != 3).astype(np.int64)
    X = G * P
    X2 = X * X
    H = (G == 1).astype(np.int64)
    xx, hh, pp = X @ X.T, H @ H.T, P @ P.T
    xP, x2P, Px, Px2 = X @ P.T, X2 @ P.T, P @ X.T, P @ X2.T
    h1 = 2 * xP - x2P - hh
    h2 = 2 * Px - Px2 - hh
    ibs0 = (x2P + Px2 - 2 * xx - h1 - h2) // 4
    with np.errstate(all="ignore"):
        kin = 0.5 - (4 * ibs0 + h1 + h2).astype(np.float64) / (4.0 * (hh + np.minimum(h1, h2)).astype(np.float64))
    i1, i2 = np.triu_indices(G.shape[0], 1)
    res = dict(I1=i1.astype(np.int32), I2=i2.astype(np.int32), KINSHIP=kin[i1, i2])
    for name, a in zip(COUNT_NAMES, (pp, hh, ibs0, h1, h2)):
        res[name] = a[i1, i2].astype(np.int32)
    return res


def direct_counts(G):
    """the five counts by their definition, pair by pair over the calls (small shapes only): (pairs, 5)"""
    G = np.asarray(G)
    i1, i2 = np.triu_indices(G.shape[0], 1)
    a, b = G[i1], G[i2]
    both = (a != 3) & (b != 3)
    het_a, het_b = both & (a == 1), both & (b == 1)
    return np.stack([both.sum(1), (het_a & het_b).sum(1), (both & (np.abs(a - b) == 2)).sum(1), (het_a & ~het_b).sum(1),
                     (het_b & ~het_a).sum(1)], axis=1).astype(np.int32)


def select(t, keep):
    return {k: v[keep] for k, v in t.items()}


def assert_same_table(got, want):
    """indices and counts equal, the kinship bit for bit (NaN and -inf at the same rows)"""
    for name in ("I1", "I2") + COUNT_NAMES:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    a, b = np.asarray(got["KINSHIP"]), np.asarray(want["KINSHIP"])
    assert a.shape == b.shape
    nan = np.isnan(a)
    np.testing.assert_array_equal(nan, np.isnan(b))
    np.testing.assert_array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))
