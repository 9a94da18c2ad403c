"""k_prodT's second split (bigsnpr_amd/csrc/prod_plan.hpp): the sample blocks that fill whole rounds of the CUs take their own,
small slab count (wgx_whole, ky_whole, cps_whole) and only the blocks beyond the last whole round keep the fine split (wgx, ky,
smaj_cps, pinned unchanged by tests/test_prod_plan_cpu.py).  prodt_slab — the text k_prodT compiles — maps a workgroup of the
one-dimensional grid to (sample block, slab, chunks); here it is walked on the CPU (tests/native/prodt_grid_ref.cpp)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))


@pytest.fixture(scope="module")
def pg():
    import prodt_grid_ref
    prodt_grid_ref.load()
    return prodt_grid_ref


def facts(n, m, **kw):
    f = dict(bits=2, n=n, m=m, pitch=(n + 511) // 512 * 128, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1,
             no_sparse=0, nvec=16, S=3, ncu=256, segmented=0)
    f.update(kw)
    return f


@pytest.mark.parametrize("S", [2, 3])
def test_headline_shape(pg, S):
    """400 000 x 1 000 000: 782 blocks on 256 CUs are three whole rounds + 14 blocks, which keep 18 slabs of 109 chunks"""
    f = facts(400000, 1000000, S=S)
    p = pg.plan(**f)
    assert (p["smaj"], p["wgx"], p["wgx_whole"], p["ky"], p["smaj_cps"]) == (1, 782, 768, 18, 109)
    assert p["ky_whole"] in (1, 2, 3)                                    # (the default: profiles/prodt_whole_rounds_ab.txt)
    assert p["cps_whole"] == -(-1954 // p["ky_whole"]) and p["ky_whole"] * p["cps_whole"] >= 1954
    assert p["workgroups"] == 768 * p["ky_whole"] + 14 * 18
    # whole-round blocks first, slab by slab; the remainder last, slab by slab
    assert pg.slab(0, **f) == (0, 0, 0, p["cps_whole"])
    assert pg.slab(767, **f) == (767, 0, 0, p["cps_whole"])
    w = 768 * p["ky_whole"]
    assert pg.slab(w - 1, **f) == (767, p["ky_whole"] - 1, (p["ky_whole"] - 1) * p["cps_whole"], 1954)
    assert pg.slab(w, **f) == (768, 0, 0, 109)
    assert pg.slab(w + 14, **f) == (768, 1, 109, 218)
    assert pg.slab(p["workgroups"] - 1, **f) == (781, 17, 17 * 109, 1954)   # the last slab is short: 101 chunks
    assert pg.check(**f) == 0
    # 304 CUs: two whole rounds, the remainder of 174 blocks keeps 12 x 163
    q = pg.plan(**dict(f, ncu=304))
    assert (q["wgx_whole"], q["ky"], q["smaj_cps"]) == (608, 12, 163) and q["workgroups"] == 608 * q["ky_whole"] + 174 * 12
    assert pg.check(**dict(f, ncu=304)) == 0


def test_slab_count_of_the_whole_rounds(pg):
    """the sweep of the profiling build (BSN_KY_WHOLE) and the int32 bound of a slab"""
    f = facts(400000, 1000000)
    for kw, cps in ((1, 1954), (2, 977), (3, 652), (18, 109)):
        p = pg.plan(ky_whole=kw, **f)
        assert (p["wgx_whole"], p["ky_whole"], p["cps_whole"]) == (768, kw, cps) and (p["ky"], p["smaj_cps"]) == (18, 109)
        assert pg.check(ky_whole=kw, **f) == 0
    assert pg.plan(ky_whole=100000, **f)["ky_whole"] == 1954             # at most one slab per chunk
    # a slab stays below 2 500 000 variants: at least ceil(m_pad / 2 500 000) slabs, whatever is asked for
    for m, least in ((2500000, 2), (2499584, 1), (4999680, 3), (6000000, 3), (12000000, 5)):
        for kw in (0, 1, 2):
            g = facts(3001, m, ncu=4, ky_whole=kw)
            p = pg.plan(**g)
            assert p["wgx_whole"] == 4 and p["ky_whole"] >= max(least, -(-p["m_pad"] // 2500000), kw), (m, kw, p)
            assert p["cps_whole"] * 512 <= 2500000 and pg.check(**g) == 0


def test_no_second_split(pg):
    """wgx_whole = 0 — the geometry as it was — for a segmented pass, with fewer blocks than CUs and off the sample-major path"""
    for f in (facts(400000, 125000, S=2, segmented=1),          # the sharded solve's segments
              facts(3001, 5003),                                # 6 blocks on 256 CUs
              facts(130000, 5003, ncu=256),                     # 254 blocks
              facts(400000, 1000000, have_smaj=0, nvec=8, S=2),
              facts(400000, 1000000, col0=64)):
        p = pg.plan(**f)
        assert (p["wgx_whole"], p["ky_whole"], p["cps_whole"]) == (0, 0, 0), f
        if p["smaj"]:
            assert p["workgroups"] == p["wgx"] * p["ky"] and pg.check(**f) == 0
            # ... in the order of the two-dimensional grid it replaces: the blocks of a slab side by side
            assert pg.slab(0, **f)[:2] == (0, 0) and pg.slab(p["wgx"] - 1, **f)[:2] == (p["wgx"] - 1, 0)
            assert pg.slab(p["wgx"], **f)[:3] == (0, 1, p["smaj_cps"])
    assert pg.plan(**facts(131072, 5003))["wgx_whole"] == 256    # exactly one round, no remainder
    assert pg.check(**facts(131072, 5003)) == 0


def test_random_facts_cover_every_chunk_once(pg):
    """every (sample block, chunk) pair in exactly one workgroup, no empty slab, none beyond 2 500 000 variants, whole rounds
    first, wgx_whole = 0 whenever the pass is segmented or has fewer blocks than CUs (pg_check walks the whole grid)"""
    rng = np.random.default_rng(20261020)
    seen_whole = seen_rest = seen_plain = seen_exact = 0
    for it in range(4000):
        big = it % 40 == 0
        n = int(rng.integers(1, 1500 if big else 20000))
        m = int(rng.integers(2000000, 7000000)) if big else int(rng.integers(1, 60000))
        col0 = int(rng.choice([0, 0, 512, 1536]))
        f = facts(n, m, col0=col0, nvec=int(rng.integers(9, 17)), S=int(rng.integers(2, 4)), has_q=int(rng.integers(0, 2)),
                  ncu=int(rng.choice([1, 2, 3, 4, 5, 7, 8, 13, 16, 64, 256])), segmented=int(rng.random() < 0.15),
                  ky_t=int(rng.choice([0, 0, rng.integers(1, 40)])), ky_whole=int(rng.choice([0, 0, rng.integers(1, 8)])))
        p = pg.plan(**f)
        assert p["smaj"] == 1, f
        assert pg.check(**f) == 0, (f, p)
        if f["segmented"] or p["wgx"] < f["ncu"]:
            assert p["wgx_whole"] == 0, (f, p)
            seen_plain += 1
        else:
            assert p["wgx_whole"] == p["wgx"] // f["ncu"] * f["ncu"] > 0, (f, p)
            seen_whole += 1
            seen_rest += p["wgx_whole"] < p["wgx"]
            seen_exact += p["wgx_whole"] == p["wgx"]
    assert min(seen_whole, seen_rest, seen_plain, seen_exact) > 100
