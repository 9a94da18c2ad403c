"""Inputs of the OADP projection tests (CPU statement and kernel): singular values, simple projections and squared norms
of ordinary samples with the edge rows first and last in the batch."""
import numpy as np

# the edge rows, in the order they are placed from the front (and, mirrored, from the back)
EDGE_KINDS = ("huge", "span", "below", "zero", "nan")


def sval(K, seed, equal_pair=False):
    """K singular values in (20, 400), descending; equal_pair: two of them equal (K >= 2)"""
    rng = np.random.default_rng(1000 + seed)
    d = np.sort(rng.uniform(20, 400, K))[::-1].copy()
    if equal_pair and K >= 2:
        d[K // 2] = d[K // 2 - 1]
    return d


def edge_rows(n):
    """{row: kind}: the first and the last rows of a batch of n"""
    rows = {}
    for t, kind in enumerate(EDGE_KINDS):
        if t < n:
            rows[t] = kind
    for t, kind in enumerate(EDGE_KINDS):
        if n - 1 - t >= len(EDGE_KINDS):
            rows[n - 1 - t] = kind
    return rows


def batch(n, d, seed):
    """(XV n x K column-major, X_norm n, {row: kind})"""
    K = d.size
    rng = np.random.default_rng(seed)
    XV = np.asfortranarray(rng.normal(size=(n, K)) * d / np.sqrt(300.0))
    X_norm = (XV ** 2).sum(axis=1) * rng.uniform(1.05, 4.0, n)
    rows = edge_rows(n)
    for i, kind in rows.items():
        l2 = float(XV[i] @ XV[i])
        if kind == "huge":      # |y|^2 > 9 d_1^2: the new sample becomes the leading direction
            X_norm[i] = 9.5 * d[0] ** 2 + l2
        elif kind == "span":    # |y|^2 = |l|^2 exactly, whatever the order |l|^2 is summed in: a row of integers
            XV[i] = np.round(XV[i]) + 1.0
            X_norm[i] = float(XV[i] @ XV[i])
        elif kind == "below":   # |y|^2 just below |l|^2 (rounding of the two passes that produce them)
            X_norm[i] = l2 * (1.0 - 1e-13)
        elif kind == "zero":
            XV[i] = 0.0
            X_norm[i] = 0.0
        elif kind == "nan":
            XV[i, K // 2] = np.nan
    return XV, X_norm, rows


def finite_rows(n, rows):
    ok = np.ones(n, dtype=bool)
    for i, kind in rows.items():
        if kind == "nan":
            ok[i] = False
    return ok
