"""The checker that the device tests of big_spLinReg / big_spLogReg share (tests/test_gpu_plr.py, tests/test_gpu_plr_shapes.py):
the device's model against the CPU statement (tests/native/plr_ref.cpp) on the same decoded matrix.

Discrete outputs (message, number of lambdas, best index, passes per lambda, non-zeros per lambda, support) are equal
exactly.  beta (relative to max|beta|), intercept, loss and loss_val (relative to the value) are within 1000 x the spread
between the statement's forward and reversed row sums ON THAT INPUT, which every check measures and prints; a spread below
one unit of fp64 rounding (2.2e-16) counts as that."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

import plr_ref as ref  # noqa: E402

EPS64 = 2.2e-16


def _raw(mod):
    """a BigSpReg as the raw arrays of the statement, chain c = a K + k in the last axis"""
    chains = [mo for mods in mod for mo in mods]
    NL = max(mo["lambda"].size for mo in chains)
    out = dict(intercept=np.array([mo["intercept"] for mo in chains]), beta=np.column_stack([mo["beta"] for mo in chains]),
               n_done=np.array([mo["iter"].size for mo in chains]), best=np.array([mo["best"] for mo in chains]),
               status=np.array([ref.MESSAGES.index(mo["message"]) for mo in chains]))
    for k in ("loss", "loss_val", "iter", "nb_active"):
        out[k] = [mo[k] for mo in chains]
    return out


def _same(mod, X, y, fold, K, where, **kw):
    """the device's model against the statement; the tolerance is measured from the statement's two orders"""
    f = ref.fit(X, y, fold, K, **kw)
    r = ref.fit(X, y, fold, K, reverse=True, **kw)
    got = _raw(mod)
    for k in ("status", "n_done", "best"):
        assert np.array_equal(f[k], r[k]), (where, k)
        assert np.array_equal(got[k], f[k]), (where, k, got[k], f[k])
    bmax = np.abs(f["beta"]).max()
    sb = max(np.abs(f["beta"] - r["beta"]).max() / bmax, EPS64) if bmax > 0 else EPS64
    si = max(np.abs(f["intercept"] / r["intercept"] - 1).max(), EPS64)
    db = np.abs(got["beta"] - f["beta"]).max() / (bmax if bmax > 0 else 1.0)
    di = np.abs(got["intercept"] / f["intercept"] - 1).max()
    sl = sv = dl = dv = 0.0
    for c in range(f["n_done"].size):
        d = f["n_done"][c]
        assert np.array_equal(got["iter"][c], f["iter"][:d, c]), (where, c, got["iter"][c], f["iter"][:d, c])
        assert np.array_equal(got["nb_active"][c], f["nb_active"][:d, c]), (where, c)
        sl = max(sl, np.abs(f["loss"][:d, c] / r["loss"][:d, c] - 1).max())
        sv = max(sv, np.abs(f["loss_val"][:d, c] / r["loss_val"][:d, c] - 1).max())
        dl = max(dl, np.abs(got["loss"][c] / f["loss"][:d, c] - 1).max())
        dv = max(dv, np.abs(got["loss_val"][c] / f["loss_val"][:d, c] - 1).max())
    sl, sv = max(sl, EPS64), max(sv, EPS64)
    print("%s: beta %.3g (spread %.3g) of max|beta| %.3g, intercept %.3g (%.3g), loss %.3g (%.3g), loss_val %.3g (%.3g); "
          "status %s, n_done %s, best %s" % (where, db, sb, bmax, di, si, dl, sl, dv, sv, f["status"], f["n_done"], f["best"]))
    assert np.array_equal(got["beta"] != 0, f["beta"] != 0), where
    assert db <= 1000 * sb and di <= 1000 * si and dl <= 1000 * sl and dv <= 1000 * sv, where
    return f


def _fit(ba, family, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return (ba.big_spLinReg if family == "linear" else ba.big_spLogReg)(*a, **kw)
