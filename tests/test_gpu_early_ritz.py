"""bed_randomSVD with u, v formed and sent to the host under the last step's product pass (early Rayleigh-Ritz)
against the same solve with BSN_NO_EARLY_RITZ=1 (the order of the parent: Gram blocks, Rayleigh-Ritz step and u, v after
the pass): d, u, v, center, scale and niter must be the SAME numbers — np.array_equal, no tolerance.  The switch is read
per call.  u and v go to page-locked memory through the C entry point (bed_randomSVD page-locks only large results, and
only page-locked destinations are served early); bsn_svd_info.early_ritz says what happened: [0] guesses queued, [1] 1 if
the returned u / v came from one."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLINK = np.array([3, 2, 0, 1], dtype=np.uint8)   # genotype 0 / 1 / 2 / missing -> the .bed code


@pytest.fixture(scope="module")
def ba():
    import bigsnpr_amd
    bigsnpr_amd.load()
    return bigsnpr_amd


def payload_of(G):
    """G [n x m] in {0, 1, 2, 3 = missing} -> the .bed payload (variant-major, four samples per byte)"""
    n, m = G.shape
    nb = (n + 3) // 4
    c = np.zeros((4 * nb, m), dtype=np.uint8)
    c[:n] = PLINK[G]
    c = c.reshape(nb, 4, m)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).T.copy().ravel()


def random_genotypes(n, m, seed):
    """independent genotypes at allele frequencies 0.05 .. 0.5, 1 % missing: a flat spectrum, many block steps"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.05, 0.5, m)
    G = rng.binomial(2, f, (n, m)).astype(np.uint8)
    G[rng.random((n, m)) < 0.01] = 3
    return G


def planted(n, m, npop, seed, na="entries"):
    """every sample carries the genotypes of its population: the scaled matrix has rank npop - 1.  na = "entries": 1 % of
    the genotypes missing (the rank is then npop - 1 plus a small tail); "samples": 1 % of the samples missing altogether
    (rows of zeros after imputation: the rank stays exact)"""
    rng = np.random.default_rng(seed)
    proto = rng.integers(0, 3, (npop, m)).astype(np.uint8)
    mono = np.all(proto == proto[0], axis=0)     # a variant every population agrees on has no variance: scale 0
    proto[0, mono] = (proto[0, mono] + 1) % 3
    G = proto[rng.integers(0, npop, n)]
    if na == "entries":
        G[rng.random((n, m)) < 0.01] = 3
    else:
        G[rng.choice(n, n // 100, replace=False)] = 3
    return G


class Pinned:
    """a page-locked block of the library (bsn_host_alloc) seen as a float64 array"""

    def __init__(self, L, shape):
        from bigsnpr_amd._lib import check
        self.L, self.p = L, C.c_void_p()
        count = int(np.prod(shape))
        check(L.bsn_host_alloc(C.byref(self.p), max(4096, count * 8)))
        self.arr = np.ctypeslib.as_array(C.cast(self.p, C.POINTER(C.c_double)), shape=(count,)).reshape(shape)
        self.arr[...] = np.nan

    def take(self):
        out = self.arr.copy()
        self.arr = None
        self.L.bsn_host_free(self.p)
        return out


def solve(gb, k, ind_row=None, ind_col=None, block=0, want_u=True, want_v=True, hook=False, warm=0, warm_den=0):
    """bsn_bed_randomsvd with bed_scaleBinom's scaling inside the solve and u, v in page-locked memory"""
    from bigsnpr_amd import _lib
    from bigsnpr_amd._lib import check, f64p, i64p, ptr
    from bigsnpr_amd.bed import _args
    L = _lib.load()
    ir, ic = _args(gb, ind_row, ind_col)
    opts, info = _lib.SvdOptions(), _lib.SvdInfo()
    center, scale = np.empty(ic.size), np.empty(ic.size)
    opts.k, opts.tol, opts.block, opts.seed = k, 1e-4, block, 1
    opts.binom_scaling = 1
    opts.warm_start, opts.warm_denominator = warm, warm_den
    opts.center_out, opts.scale_out = ptr(center, f64p), ptr(scale, f64p)
    cb = None
    if hook:   # the host all-reduce hook with one rank: the sum over the ranks is what is there
        cb = _lib.ALLREDUCE_FN(lambda p, count, ctx: None)
        opts.allreduce = cb
        opts.hook_rank, opts.hook_world = 0, 1
    d = np.empty(k)
    u = Pinned(L, (k, ir.size)) if want_u else None
    v = Pinned(L, (k, ic.size)) if want_v else None
    rc = L.bsn_bed_randomsvd(gb.handle, ptr(ir, i64p), ir.size, ptr(ic, i64p), ic.size, None, None, C.byref(opts),
                             ptr(d, f64p), None if u is None else C.cast(u.p, f64p), None if v is None else C.cast(v.p, f64p),
                             C.byref(info))
    out = dict(d=d, u=None if u is None else u.take(), v=None if v is None else v.take(), center=center, scale=scale,
               niter=int(info.niter), basis=int(info.basis), block=int(info.block), converged=int(info.converged), early_ritz=[int(x) for x in info.early_ritz])
    if rc not in (0, 2):
        check(rc)
    return out


def same(a, b, what):
    for key in ("d", "u", "v", "center", "scale"):
        if a[key] is None:
            assert b[key] is None, (what, key)
        else:
            assert np.all(np.isfinite(a[key])), (what, key)
            assert np.array_equal(a[key], b[key]), (what, key, float(np.abs(a[key] - b[key]).max()))
    assert a["niter"] == b["niter"] and a["converged"] == b["converged"], (what, a["niter"], b["niter"])


def ab(monkeypatch, gb, what, **kw):
    """default, BSN_NO_EARLY_RITZ=1, default again (the handle's cached statistics serve the later two)"""
    monkeypatch.delenv("BSN_NO_EARLY_RITZ", raising=False)
    on = solve(gb, **kw)
    monkeypatch.setenv("BSN_NO_EARLY_RITZ", "1")
    off = solve(gb, **kw)
    monkeypatch.delenv("BSN_NO_EARLY_RITZ")
    again = solve(gb, **kw)
    print("%s: niter %d, basis %d, converged %d, early_ritz %s / %s / %s" % (what, on["niter"], on["basis"], on["converged"], on["early_ritz"],
                                                                  off["early_ritz"], again["early_ritz"]))
    same(on, off, what)
    same(again, off, what + " (again)")
    assert off["early_ritz"] == [0, 0], (what, off["early_ritz"])
    assert again["early_ritz"] == on["early_ritz"], (what, on["early_ritz"], again["early_ritz"])
    return on, off


@pytest.fixture(scope="module")
def payload_a():
    return payload_of(random_genotypes(1500, 4000, 11))


def test_many_steps_two_column_chunks(ba, payload_a, monkeypatch):
    """(a) 1 500 x 4 000, k = 20, block 8: k > 16 puts two column chunks through the u / v kernels; the flat spectrum takes
    many steps, each with a guess that is dropped, and fills the basis (thick restart)"""
    gb = ba.bed.from_payload(payload_a, 1500, 4000)
    on, _ = ab(monkeypatch, gb, "(a)", k=20, block=8)
    assert on["converged"] == 1 and on["niter"] > 4
    # a thick restart: the info has no restart count, but every step of this full-rank matrix adds a whole block, so a
    # basis at exit smaller than the blocks the steps added is one that was compressed on the way
    assert on["block"] == 8 and on["basis"] < 8 * on["niter"], (on["basis"], on["niter"])
    assert on["early_ritz"][1] == 1 and on["early_ritz"][0] >= 2, on["early_ritz"]


def test_planted_rank3(ba, monkeypatch):
    """(b) four populations (rank 3 plus the tail of 1 % missing genotypes), 3 000 x 900, k = 3: the basis holds k vectors
    from the first step on, so the first step already guesses and every step of the solve does.  The solve itself takes
    three steps with the switch set or unset (measured): its start block is random — the warm start needs 32 768 variants
    or more — and Ritz pairs on a random block cannot meet the tolerance, so no 900-variant matrix ends at its first
    step.  The path "the first guess is kept, none dropped" is pinned by tests/native/early_ritz_check.cpp (one-step
    case), where the backend's warm start runs on the whole matrix."""
    n, m = 3000, 900
    gb = ba.bed.from_payload(payload_of(planted(n, m, 4, 12)), n, m)
    on, _ = ab(monkeypatch, gb, "(b)", k=3)
    assert on["converged"] == 1
    assert on["early_ritz"] == [on["niter"], 1], (on["early_ritz"], on["niter"])   # a guess at every step, the first included


def test_row_subset(ba, payload_a, monkeypatch):
    """(c) (a)'s matrix over 700 of its samples (not a multiple of 256)"""
    gb = ba.bed.from_payload(payload_a, 1500, 4000)
    rows = np.sort(np.random.default_rng(13).choice(1500, 700, replace=False))
    on, _ = ab(monkeypatch, gb, "(c)", k=20, block=8, ind_row=rows)
    assert on["converged"] == 1
    assert on["early_ritz"][1] == 1, on["early_ritz"]


def test_rank_deficient_takes_the_careful_path(ba, monkeypatch):
    """(d) rank 12 exactly (13 populations, missing values as whole samples), k = 20: the panels run out of directions, the
    last step is orthonormalised on the careful path and its guess is dropped"""
    n, m = 1200, 1600
    gb = ba.bed.from_payload(payload_of(planted(n, m, 13, 14, na="samples")), n, m)
    on, _ = ab(monkeypatch, gb, "(d)", k=20)
    assert on["early_ritz"][1] == 0, on["early_ritz"]
    # (beyond the rank: below what the driver itself calls zero, theta < 1e-10 theta_1)
    assert np.all(on["d"][12:] < 1e-4 * on["d"][0]) and on["d"][11] > 1e-3 * on["d"][0], on["d"]


def test_null_outputs(ba, payload_a, monkeypatch):
    """(e) u only, v only, neither"""
    gb = ba.bed.from_payload(payload_a, 1500, 4000)
    full = solve(gb, k=20, block=8)
    for want_u, want_v in ((True, False), (False, True), (False, False)):
        on, _ = ab(monkeypatch, gb, "(e) u %d v %d" % (want_u, want_v), k=20, block=8, want_u=want_u, want_v=want_v)
        assert np.array_equal(on["d"], full["d"])
        if want_u:
            assert np.array_equal(on["u"], full["u"])
        if want_v:
            assert np.array_equal(on["v"], full["v"])
        if not (want_u or want_v):
            assert on["early_ritz"] == [0, 0], on["early_ritz"]   # nothing to form early


def test_host_allreduce_hook_keeps_the_parents_order(ba, payload_a, monkeypatch):
    """(f) the host all-reduce hook with one rank: no early step at all"""
    gb = ba.bed.from_payload(payload_a, 1500, 4000)
    on, _ = ab(monkeypatch, gb, "(f)", k=20, block=8, hook=True)
    assert on["early_ritz"] == [0, 0], on["early_ritz"]
