"""Shared by test_ibd_cpu.py and test_gpu_ibd.py: the NumPy restatement of DESIGN.md 3.5p (moments, IBS counts, estimate),
the pruning rule of indep_pairwise over a dense r^2, fixed-seed shapes and the comparison of two tables.  Not a test
module."""
import numpy as np

import king_cases as kc

IBS_NAMES = ("IBS0", "IBS1", "IBS2")
EST_NAMES = ("Z0", "Z1", "Z2", "PI_HAT", "DST")


def variant_counts(G, freq=None):
    """m x 3 counts n0, n1, n2 of the called genotypes of every variant among the rows `freq` (None: all)"""
    G = np.asarray(G)
    if freq is not None:
        G = G[np.asarray(freq).astype(bool)]
    return np.stack([(G == c).sum(axis=0) for c in (0, 1, 2)], axis=1).astype(np.int64)


def numpy_terms(counts):
    """(a, used): the five terms of every variant (m x 5; 0 where unused) from its counts, by the formulas of 3.5p"""
    c = np.asarray(counts, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        Na = 2 * (c[:, 0] + c[:, 1] + c[:, 2])
        p = (c[:, 1] + 2 * c[:, 2]) / Na
        q = 1 - p
        used = (Na > 3) & (p > 0) & (q > 0)
        f2 = Na * Na / ((Na - 1) * (Na - 2))
        f3 = f2 * Na / (Na - 3)
        x, y = p * Na, q * Na
        x1 = (x - 1) / x
        x2 = x1 * (x - 2) / x
        y1 = (y - 1) / y
        y2 = y1 * (y - 2) / y
        a = np.stack([2 * p ** 2 * q ** 2 * x1 * y1 * f3,
                      4 * p * q * f3 * (p ** 2 * x2 + q ** 2 * y2),
                      f3 * (q ** 4 * y2 * (y - 3) / y + p ** 4 * x2 * (x - 3) / x + 4 * p ** 2 * q ** 2 * x1 * y1),
                      2 * p * q * f2 * (p * x1 + q * y1),
                      f2 * (p ** 3 * x2 + q ** 3 * y2 + p ** 2 * q * x1 + p * q ** 2 * y1)], axis=1)
    a[~used] = 0
    return a, used


def numpy_estimate(ibs, E):
    """k x 5 (Z0, Z1, Z2, PI_HAT, DST) from rows of (IBS0, IBS1, IBS2) and the five moments, in the stated order"""
    ibs = np.asarray(ibs, dtype=np.int64).reshape(-1, 3)
    E00, E01, E02, E11, E12 = (np.float64(v) for v in E)
    i0, i1, i2 = (ibs[:, q].astype(np.float64) for q in range(3))
    with np.errstate(all="ignore"):
        S = (ibs[:, 0] + ibs[:, 1] + ibs[:, 2]).astype(np.float64)
        r = 1.0 / S
        z0 = i0 * r / E00
        z1 = (i1 * r - z0 * E01) / E11
        z2 = i2 * r - z0 * E02 - z1 * E12
        for hit, val in ((lambda: z0 > 1, (1.0, 0.0, 0.0)), (lambda: z1 > 1, (0.0, 1.0, 0.0)), (lambda: z2 > 1, (0.0, 0.0, 1.0))):
            h = hit()
            z0, z1, z2 = np.where(h, val[0], z0), np.where(h, val[1], z1), np.where(h, val[2], z2)
        h = z0 < 0
        s = z1 + z2
        z1, z2, z0 = np.where(h, z1 / s, z1), np.where(h, z2 / s, z2), np.where(h, 0.0, z0)
        h = z1 < 0
        s = z0 + z2
        z0, z2, z1 = np.where(h, z0 / s, z0), np.where(h, z2 / s, z2), np.where(h, 0.0, z1)
        h = z2 < 0
        s = z0 + z1
        z0, z1, z2 = np.where(h, z0 / s, z0), np.where(h, z1 / s, z1), np.where(h, 0.0, z2)
        pi = z1 * 0.5 + z2
        h = pi * pi <= z2
        z0 = np.where(h, (1.0 - pi) * (1.0 - pi), z0)
        z1 = np.where(h, 2.0 * pi * (1.0 - pi), z1)
        z2 = np.where(h, pi * pi, z2)
        dst = (i2 + 0.5 * i1) * r
    return np.stack([z0, z1, z2, pi, dst], axis=1)


def numpy_table(G, freq=None):
    """I1, I2, the IBS counts by their definition through int64 matrix products, E (NumPy's own order of summation) and
    n_used"""
    G = np.asarray(G).astype(np.int64)
    n = G.shape[0]
    P = (G != 3).astype(np.int64)
    hom0, het, hom2 = ((G == c).astype(np.int64) for c in (0, 1, 2))
    hom = hom0 + hom2
    nsnp = P @ P.T
    ibs0 = hom0 @ hom2.T + hom2 @ hom0.T
    ibs1 = het @ hom.T + hom @ het.T
    i1, i2 = np.triu_indices(n, 1)
    a, used = numpy_terms(variant_counts(G, freq))
    res = dict(I1=i1.astype(np.int32), I2=i2.astype(np.int32), IBS0=ibs0[i1, i2].astype(np.int32), IBS1=ibs1[i1, i2].astype(np.int32),
               IBS2=(nsnp - ibs0 - ibs1)[i1, i2].astype(np.int32))
    res["n_used"] = int(used.sum())
    res["E"] = a[used].sum(axis=0) / float(used.sum()) if used.any() else np.full(5, np.nan)
    return res


def assert_same_doubles(a, b, name=""):
    """equal by bytes, NaN at the same places"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, name
    nan = np.isnan(a)
    np.testing.assert_array_equal(nan, np.isnan(b), err_msg=name)
    np.testing.assert_array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64), err_msg=name)


def assert_same_table(got, want):
    """indices and counts equal, the doubles (the estimate and E) equal by bytes, n_used equal"""
    for name in ("I1", "I2") + IBS_NAMES:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    for name in EST_NAMES + ("E",):
        assert_same_doubles(got[name], want[name], name)
    assert got["n_used"] == want["n_used"]


def small_matrix():
    """37 x 301, 5 % missing, sample 11 entirely missing"""
    G = kc.random_codes(37, 301, 0.05, seed=20261020)
    G[11] = 3
    return G


def small_freq():
    """a frequency mask of 6 samples: some variants are monomorphic among them, and sample 11 has no call"""
    f = np.zeros(37, dtype=bool)
    f[[1, 4, 11, 20, 21, 36]] = True
    return f


def prune_rule(r2, maf, chrom, window, thr_r2):
    """the rule of indep_pairwise from a dense m x m r^2: per chromosome, positions in the order given, the pairs i < j with
    j - i < window whose r^2 is above thr_r2 (NaN is not), walked by prune_walk.  Returns the kept mask."""
    from bigsnpr_amd.ibd import prune_walk
    r2, maf, chrom = np.asarray(r2, dtype=np.float64), np.asarray(maf, dtype=np.float64), np.asarray(chrom)
    keep = np.ones(maf.size, dtype=bool)
    seen = []
    for c in chrom.tolist():
        if c not in seen:
            seen.append(c)
    for c in seen:
        where = np.flatnonzero(chrom == c)
        sub = r2[np.ix_(where, where)]
        pi, pj = np.triu_indices(where.size, 1)
        with np.errstate(invalid="ignore"):
            ok = (pj - pi < window) & (sub[pi, pj] > thr_r2)
        keep[where] = prune_walk(pi[ok], pj[ok], maf[where])
    return keep
