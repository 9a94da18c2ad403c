"""The solve plan of bsn_bed_randomsvd (bigsnpr_amd/csrc/svd_plan.hpp: plan_solve, plan_resolve, needs_resolve, on_prodT),
pinned on the CPU through tests/native.  The expected values are literal: they were written from the arithmetic of the entry
point as it stood before the plan was moved out of it (block and digit slices from tol and k, the precision schedule from
vec_floor, the start grid, the warm start, which second copy of the image a solve wants), one row on either side of every
threshold."""
import ctypes as C
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from svd_plan_calls import PLAN, needs_resolve, on_prodT, plan, resolve  # noqa: E402  (its BASE: the facts a row does not name)


@pytest.fixture(scope="module")
def nt():
    import build_native
    return C.CDLL(build_native.build())


# (facts that differ from BASE) -> (block, slices_base = digits of the products, slices_max, vec_floor, slices_start)
PLAN_TABLE = [
    # --- the default tolerance: 16-bit products (1.2 * 2^-16 = 1.83e-5 <= tol / 4), 8 vectors in one column block or 16 in two;
    #     two when 4 k >= 7 * 8 and the warm start runs
    (dict(), (16, 2, 3, 1e-7, 1)),
    (dict(tol=0.0), (16, 2, 3, 1e-7, 1)),                       # 0 -> 1e-4
    (dict(k=14), (16, 2, 3, 1e-7, 1)),
    (dict(k=13), (8, 2, 3, 1e-7, 1)),
    # the warm start needs 16 384 variants in the leading 1/16 over all ranks
    (dict(m_total=262143), (8, 2, 3, 1e-7, 1)),
    (dict(m_total=262144), (16, 2, 3, 1e-7, 1)),
    (dict(m_total=524287, warm_denominator=32), (8, 2, 3, 1e-7, 1)),
    (dict(m_total=524288, warm_denominator=32), (16, 2, 3, 1e-7, 1)),
    (dict(m_total=262144, warm_denominator=1), (16, 2, 3, 1e-7, 1)),   # below 2 -> 16
    (dict(warm_start=-1), (8, 2, 3, 1e-7, 1)),
    (dict(warm_start=3), (16, 2, 3, 1e-7, 1)),
    # --- tighter tolerances: the smallest S with 1.2 * 2^(-8 S) <= tol / 4; b1 = 16 // S, b2 = 32 // S
    (dict(tol=7.4e-5, k=10), (8, 2, 3, 1e-7, 1)),
    (dict(tol=7.3e-5, k=10), (10, 3, 3, 1e-7, 1)),              # b1 = 5: 40 >= 35
    (dict(tol=1e-5, k=9), (10, 3, 3, 1e-7, 1)),                 # 36 >= 35
    (dict(tol=1e-5, k=8), (5, 3, 3, 1e-7, 1)),                  # 32 < 35
    (dict(tol=2.9e-7), (10, 3, 3, 1e-7, 1)),
    (dict(tol=2.8e-7), (8, 4, 4, 1e-7, 1)),                     # 4 * 1.2 * 2^-24 = 2.86e-7
    (dict(tol=1e-8), (8, 4, 4, 1e-7, 1)),
    (dict(tol=1.2e-9), (8, 4, 4, 1e-7, 1)),
    (dict(tol=1.1e-9), (6, 5, 5, 1e-7, 1)),                     # 4 * 1.2 * 2^-32 = 1.118e-9
    (dict(tol=4.4e-12), (6, 5, 5, 1e-7, 1)),
    (dict(tol=4.3e-12), (5, 6, 6, 1e-7, 1)),                    # 4 * 1.2 * 2^-40 = 4.366e-12
    (dict(tol=1e-12), (5, 6, 6, 1e-7, 1)),
    (dict(tol=1.8e-14), (5, 6, 6, 1e-7, 1)),
    (dict(tol=1.7e-14), (4, 7, 7, 1e-7, 1)),                    # 4 * 1.2 * 2^-48 = 1.705e-14
    (dict(tol=1e-30), (4, 7, 7, 1e-7, 1)),                      # never more than 56 bits
    # --- a block chosen by the caller gets as many digits as its column blocks hold anyway
    (dict(block=1), (1, 7, 7, 1e-7, 1)),
    (dict(block=2), (2, 7, 7, 1e-7, 1)),
    (dict(block=3), (3, 5, 5, 1e-7, 1)),
    (dict(block=5), (5, 3, 3, 1e-7, 1)),
    (dict(block=6), (6, 2, 3, 1e-7, 1)),
    (dict(block=8), (8, 2, 3, 1e-7, 1)),
    (dict(block=16), (16, 2, 3, 1e-7, 1)),
    (dict(block=17), (16, 2, 3, 1e-7, 1)),
    (dict(block=40), (16, 2, 3, 1e-7, 1)),
    # --- digits fixed by the caller: no schedule unless a floor is named too, and the start block on the grid of the rest
    (dict(slices=2), (16, 2, 2, 0.0, 0)),
    (dict(slices=2, vec_floor=1e-7), (16, 2, 3, 1e-7, 0)),
    (dict(slices=2, block=8), (8, 2, 2, 0.0, 0)),
    (dict(slices=7), (4, 7, 7, 0.0, 0)),
    # --- the floor wanted for the vectors: digits of the early steps up to the smallest S with 1.2 * 2^(-8 S) <= floor
    (dict(vec_floor=1.9e-5), (16, 2, 2, 1.9e-5, 1)),
    (dict(vec_floor=1.8e-5), (16, 2, 3, 1.8e-5, 1)),
    (dict(vec_floor=7.2e-8), (16, 2, 3, 7.2e-8, 1)),
    (dict(vec_floor=7.1e-8), (16, 2, 4, 7.1e-8, 1)),            # 1.2 * 2^-24 = 7.15e-8
    (dict(vec_floor=-1.0), (16, 2, 2, 0.0, 1)),
    # --- the switches
    (dict(env_vec_floor_set=1, env_vec_floor=-1.0), (16, 2, 2, 0.0, 1)),
    (dict(env_vec_floor_set=1, env_vec_floor=1e-9), (16, 2, 4, 1e-9, 1)),
    (dict(env_vec_floor_set=1, env_vec_floor=1e-9, vec_floor=-1.0), (16, 2, 4, 1e-9, 1)),
    (dict(env_vec_floor_set=0, env_vec_floor=1e-9), (16, 2, 3, 1e-7, 1)),
    (dict(env_start_slices_set=1, env_start_slices=0), (16, 2, 3, 1e-7, 0)),
    (dict(env_start_slices_set=1, env_start_slices=2, slices=2), (16, 2, 2, 0.0, 2)),
]


@pytest.mark.parametrize("kw,want", PLAN_TABLE, ids=[",".join("%s=%s" % kv for kv in kw.items()) or "base" for kw, _ in PLAN_TABLE])
def test_plan_solve(nt, kw, want):
    p = plan(nt, **kw)
    assert (p["block"], p["slices_base"], p["slices_max"], p["vec_floor"], p["slices_start"]) == want
    assert p["op_slices"] == p["slices_base"]
    assert p["resid_floor"] == 1.2 * 2.0 ** (-8 * p["op_slices"])
    assert p["k"] == kw.get("k", 20) and p["tol"] == (kw.get("tol") or 1e-4)


def test_plain_options(nt):
    assert [plan(nt, warm_start=w)["warm"] for w in (0, -1, -5, 1, 2, 7)] == [2, 0, 0, 1, 2, 7]
    assert [plan(nt, warm_start=w)["warm_on"] for w in (0, -1, 1)] == [1, 0, 1]
    assert plan(nt, m_total=262143)["warm_on"] == 0 and plan(nt, m_total=262143)["warm"] == 2   # (the backend declines, the option stands)
    assert [plan(nt, max_restarts=r)["max_restarts"] for r in (0, -1, 3)] == [100, -1, 3]
    assert [plan(nt, seed=s)["seed"] for s in (0, 1, 77, 4294967295)] == [1, 1, 77, 4294967295]
    assert [plan(nt, max_basis=b)["max_basis"] for b in (0, 120)] == [0, 120]
    assert [plan(nt, verbose=v)["verbose"] for v in (0, 2)] == [0, 2]
    # the noise gain of standardised columns: only with the scaling inside the solve AND the switch
    assert plan(nt)["noise_gain"] == 0 and plan(nt, fused=1)["noise_gain"] == 0 and plan(nt, env_zq_split=1)["noise_gain"] == 0
    assert plan(nt, fused=1, env_zq_split=1)["noise_gain"] == math.sqrt(2000.0)
    assert plan(nt, fused=1, env_zq_split=1, n=123457)["noise_gain"] == math.sqrt(123457.0)


def test_second_copy(nt):
    """wants_smaj: passes of more than one column block at the widest step, whole 512-variant chunks, at least 4 096
    variants; tile_ok: one column block at the base digits, whole 64-variant tiles, at least 4 096 variants"""
    def both(**kw):
        p = plan(nt, **kw)
        return int(p["wants_smaj"]), int(p["tile_ok"])
    assert both() == (1, 0)                                # 16 x 3 digit columns; 16 x 2 = 32 > 16
    assert both(k=10) == (1, 1)                            # 8 x 3 = 24 > 16, 8 x 2 = 16
    assert both(m=4096) == (1, 0) and both(m=4095) == (0, 0)
    assert both(k=10, m=4096) == (1, 1) and both(k=10, m=4095) == (0, 0)
    assert both(k=10, col0=512) == (1, 1) and both(k=10, col0=576) == (0, 1)
    assert both(k=10, col0=64) == (0, 1) and both(k=10, col0=96) == (0, 0)
    assert both(k=10, cols_contig=0) == (0, 0) and both(cols_contig=0) == (0, 0)
    # block * slices_max = 16 / 17 (one digit, no schedule)
    assert both(slices=1, block=16) == (0, 1)
    p = plan(nt, slices=1, block=16, vec_floor=1e-3)
    assert (p["slices_base"], p["slices_max"]) == (1, 2) and (int(p["wants_smaj"]), int(p["tile_ok"])) == (1, 1)   # 16 / 32
    assert both(slices=2, block=8) == (0, 1) and both(slices=3, block=5) == (0, 1)       # 16, 15
    assert both(slices=3, block=6) == (1, 0)                                             # 18, 18
    # block * slices_base = 16 / 17: 17 is prime, so the neighbours are 16 (8 x 2) and 18 (9 x 2)
    assert both(slices=2, block=9) == (1, 0)


def test_on_prodT(nt):
    """bsn_svd_info::tiled == 2: more than one and at most three column blocks, on whole 512-variant chunks (no size limit)"""
    p = plan(nt)
    assert p["block"] * p["slices_max"] == 48 and on_prodT(nt, p) == 1
    p49 = dict(p, block=7, slices_max=7)
    assert on_prodT(nt, p49) == 0 and on_prodT(nt, dict(p, block=12, slices_max=4)) == 1      # 49 / 48
    assert on_prodT(nt, dict(p, block=16, slices_max=1)) == 0 and on_prodT(nt, dict(p, block=17, slices_max=1)) == 1   # 16 / 17
    assert on_prodT(nt, p, col0=512) == 1 and on_prodT(nt, p, col0=576) == 0 and on_prodT(nt, p, col0=64) == 0
    assert on_prodT(nt, p, cols_contig=0) == 0
    assert on_prodT(nt, p, m=4095) == 1 and plan(nt, m=4095)["wants_smaj"] == 0               # the two differ here: kept as found
    q = resolve(nt, p)
    assert q["block"] * q["slices_max"] == 28 and on_prodT(nt, q) == 1


@pytest.mark.parametrize("kw", [dict(), dict(k=10), dict(block=3), dict(block=1), dict(tol=1e-8), dict(vec_floor=7.1e-8)])
def test_plan_resolve(nt, kw):
    p = plan(nt, **kw)
    q = resolve(nt, p)
    assert (q["slices_base"], q["slices_max"], q["op_slices"]) == (7, 7, 7)
    assert q["vec_floor"] == 0.0 and q["block"] == min(p["block"], 4) and q["resid_floor"] == 1.2 * 2.0 ** -56
    rest = [k for k in PLAN if k not in ("slices_base", "slices_max", "op_slices", "vec_floor", "block", "resid_floor")]
    assert [q[k] for k in rest] == [p[k] for k in rest]


def test_needs_resolve(nt):
    def need(exhausted, resid, below, p=None, **kw):
        return needs_resolve(nt, exhausted, resid, below, p, **kw)
    assert need(0, 0.0, 0) == 0
    assert need(1, 1.1e-9, 0) == 1 and need(1, 1e-9, 0) == 0 and need(0, 1.0, 0) == 0      # an INEXACT exhaustion
    assert need(0, 0.0, 1) == 1 and need(1, 1e-12, 3) == 1                                 # triplets below the resolution
    assert need(1, 1.0, 2, slices=2) == 0 and need(0, 0.0, 2, slices=7) == 0               # the caller fixed the digits
    assert need(1, 1.0, 2, block=1) == 0                                                   # 56 bits already
    assert need(1, 1.0, 2, block=3) == 1 and need(1, 1.0, 0, tol=1e-12) == 1               # 40 and 48 bits
    assert need(1, 1.0, 2, p=resolve(nt, plan(nt))) == 0                                   # no third solve
