"""k_cprod's one-dimensional grid (bigsnpr_amd/csrc/prod_plan.hpp: plan_cprod, cprod_slab): the blocks of variants that fill
whole rounds of ncu x resident workgroups keep one workgroup over all 512-sample chunks; the blocks beyond the last whole round
are cut along the samples into slabs, whose partial sums k_cprod_final adds.  cprod_slab — the text k_cprod compiles — maps a
workgroup to (block, slab, chunks); here the whole grid is walked on the CPU (tests/native/cprod_grid_ref.cpp)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))


@pytest.fixture(scope="module")
def cg():
    import cprod_grid_ref
    cprod_grid_ref.load()
    return cprod_grid_ref


def test_headline_shape(cg):
    """400 000 x 1 000 000 on 256 CUs: 1 954 blocks of 512 variants are seven whole rounds + 162 blocks"""
    for NB in (2, 3):
        f = cg.facts(400000, 1000000, NB)
        p = cg.plan(**f)
        assert (p["blocks"], p["blocks_whole"], p["nchunks"], p["m_rem"]) == (1954, 1792, 782, 1000000 - 1792 * 512), p
        # two column blocks: 162 x 11 = 1 782 workgroups, 6.96 rounds; three (half as many slabs again to pay for): 486, 1.9
        s, cps = ((11, 72) if NB == 2 else (3, 261))
        assert (p["slabs"], p["cps"]) == (s, cps), p
        assert p["workgroups"] == 1792 + 162 * s
        assert p["partial_words"] == s * 2 * p["m_rem"] * 16 * NB
        # whole-round blocks first, over all chunks; the remainder last, slab by slab
        assert cg.slab(0, **f) == (0, 0, 0, 782) and cg.slab(1791, **f) == (1791, 0, 0, 782)
        assert cg.slab(1792, **f) == (1792, 0, 0, cps) and cg.slab(1792 + 161, **f) == (1953, 0, 0, cps)
        assert cg.slab(1792 + 162, **f) == (1792, 1, cps, 2 * cps)
        assert cg.slab(p["workgroups"] - 1, **f) == (1953, s - 1, (s - 1) * cps, 782)    # the last slab is short
        assert cg.check(**f) == 0
    # one column block: 3 907 blocks of 256 variants, three resident per CU: five rounds of 768 + 67 blocks
    f = cg.facts(400000, 1000000, 1, resident=3)
    p = cg.plan(**f)
    assert (p["blocks"], p["blocks_whole"], p["m_rem"], p["slabs"]) == (3907, 3840, 1000000 - 3840 * 256, 11), p
    assert p["workgroups"] == 3840 + 67 * 11 and cg.check(**f) == 0
    # complete data: one plane, half the partial sums
    f1 = cg.facts(400000, 1000000, 3, nplane=1)
    assert cg.plan(**f1)["partial_words"] == cg.plan(**f1)["slabs"] * cg.plan(**f1)["m_rem"] * 48 and cg.check(**f1) == 0


def test_warm_start_launch(cg):
    """62 500 variants: 245 one-block workgroups where a CU holds two — all remainder, two slabs of 391 chunks fill 490 of the
    512 places (where it holds three: three slabs, 735 of 768); with two column blocks (123 workgroups of 512 variants, one
    per CU) again two slabs"""
    f = cg.facts(400000, 62500, 1)
    p = cg.plan(**f)
    assert (p["blocks"], p["blocks_whole"], p["slabs"], p["cps"], p["m_rem"], p["workgroups"]) == (245, 0, 2, 391, 62500, 490), p
    assert cg.slab(0, **f) == (0, 0, 0, 391) and cg.slab(245, **f) == (0, 1, 391, 782) and cg.slab(489, **f) == (244, 1, 391, 782)
    assert cg.check(**f) == 0
    assert cg.plan(**cg.facts(400000, 62500, 1, resident=3))["slabs"] == 3
    f = cg.facts(400000, 62500, 2)
    p = cg.plan(**f)
    assert (p["blocks"], p["blocks_whole"], p["slabs"], p["workgroups"]) == (123, 0, 2, 246), p
    assert cg.check(**f) == 0


def test_old_geometry(cg):
    """one workgroup per block where the blocks are whole rounds, where there is a single chunk, where the split would not pay
    and under the switch"""
    for f in (cg.facts(400000, 256 * 512, 3),                   # exactly one round
              cg.facts(400000, 3 * 256 * 512 - 5, 2),           # three rounds, the last block ragged
              cg.facts(512, 1000000, 3),                        # a single chunk
              cg.facts(400000, 1000000, 3, one_split=1),
              cg.facts(400000, 62500, 1, one_split=1),
              cg.facts(400000, 125000, 2),                      # 245 of 256 places taken: no count pays
              cg.facts(400000, 125000, 1, resident=3),          # 489 blocks: every CU has one, the launch is bound by HBM
              cg.facts(400000, 1000000, 1, resident=2),         # 323 blocks beyond seven rounds: no CU stands empty
              cg.facts(2000, 255 * 512, 3)):                    # 255 of 256 places taken: nothing to gain
        p = cg.plan(**f)
        assert (p["blocks_whole"], p["slabs"], p["cps"], p["m_rem"], p["partial_words"]) == (p["blocks"], 0, 0, 0, 0), (f, p)
        assert p["workgroups"] == p["blocks"] and cg.check(**f) == 0
        assert cg.slab(p["blocks"] - 1, **f) == (p["blocks"] - 1, 0, 0, p["nchunks"])


def test_slab_count_of_the_caller(cg):
    """BSN_CPROD_SLABS: whole chunks per slab, at most one slab per chunk, one slab is the old geometry"""
    for want, slabs, cps in ((4, 4, 3), (3, 3, 4), (10, 10, 1), (6, 5, 2), (500, 10, 1)):
        f = cg.facts(4645, 10 * 512 - 37, 3, ncu=4, slabs=want)      # 10 chunks; two rounds of 4 and two blocks
        p = cg.plan(**f)
        assert (p["blocks"], p["blocks_whole"], p["slabs"], p["cps"], p["m_rem"]) == (10, 8, slabs, cps, 2 * 512 - 37), (want, p)
        assert cg.check(**f) == 0
    f = cg.facts(4645, 10 * 512 - 37, 3, ncu=4, slabs=1)
    assert cg.plan(**f)["blocks_whole"] == 10 and cg.check(**f) == 0
    assert cg.plan(**cg.facts(4645, 11 * 512 - 37, 3, ncu=4))["blocks_whole"] == 11      # (the rule: too few samples to pay)
    assert cg.plan(**cg.facts(20000, 9 * 512, 2, ncu=4))["slabs"] == 4                   # one block on four CUs, 40 chunks: it pays


def test_random_shapes_cover_every_chunk_once(cg):
    """every (block, chunk) pair in exactly one workgroup, slabs contiguous and non-empty, whole rounds first, every word of the
    partial region written once and the region as large as the planner says (cg_check walks the whole grid)"""
    rng = np.random.default_rng(20261020)
    seen_split = seen_all_rest = seen_old = seen_short = seen_one_chunk_slab = 0
    for it in range(600):
        NB = int(rng.integers(1, 4))
        n = int(rng.integers(1, 30000))
        ncu = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 13, 16, 64, 256]))
        resident = int(rng.integers(1, 4))
        m = int(rng.integers(1, 40 * ncu * resident * 64 + 3000))
        f = cg.facts(n, m, NB, nplane=int(rng.integers(1, 3)), ncu=ncu, resident=resident, one_split=int(rng.random() < 0.1),
                     slabs=int(rng.choice([0, 0, 0, rng.integers(1, 70)])))
        p = cg.plan(**f)
        assert cg.check(**f) == 0, (f, p)
        if p["slabs"]:
            seen_split += p["blocks_whole"] > 0
            seen_all_rest += p["blocks_whole"] == 0
            seen_short += p["slabs"] * p["cps"] > p["nchunks"]
            seen_one_chunk_slab += p["cps"] == 1
        else:
            seen_old += 1
    assert min(seen_split, seen_all_rest, seen_old, seen_short) > 30 and seen_one_chunk_slab > 0, (
        seen_split, seen_all_rest, seen_old, seen_short, seen_one_chunk_slab)
