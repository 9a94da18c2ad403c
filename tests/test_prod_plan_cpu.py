"""The launch geometry of the streaming products (bigsnpr_amd/csrc/prod_plan.hpp: plan_prod) and the instance of k_cprod /
k_prod / k_prodT a launch takes (choose_cprod, choose_prod, choose_prodT), pinned on the CPU through tests/native.  The
expected plans are literal: they were printed by the lines of prod_planes as they stood before the geometry was moved out of
it (copied verbatim into a host program and swept against plan_prod: 58.8 million cases, no difference,
profiles/prod_dispatch_refactor.txt), the kernel records were written from its launch ladders."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

FIELDS = ("bits", "n", "m", "pitch", "col0", "cols_contig", "have_smaj", "mode", "raw_na", "has_q", "no_sparse", "nvec", "S", "ncu",
          "segmented", "ky", "ky_t")
NONE, PITCH_LIMIT, NOTHING_QUEUED = range(3)   # ProdRefusal


@pytest.fixture(scope="module")
def nt():
    import build_native
    lib = C.CDLL(build_native.build())
    lib.nt_prod_plan.argtypes = [C.c_void_p, C.c_void_p]
    lib.nt_choose_cprod.argtypes = [C.c_void_p, C.c_void_p]
    lib.nt_choose_prod.argtypes = [C.c_int] * 6 + [C.c_void_p]
    lib.nt_choose_prodT.argtypes = [C.c_int] * 5 + [C.c_void_p]
    lib.nt_prod_limits.argtypes = [C.c_void_p]
    return lib


def plan(nt, **kw):
    assert set(kw) <= set(FIELDS)
    f = np.array([kw.get(k, 0) for k in FIELDS], dtype=np.int64)
    out = np.zeros(9, dtype=np.int64)
    nt.nt_prod_plan(f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def prod_kernel(nt, *a):
    out = np.zeros(6, dtype=np.int32)
    nt.nt_choose_prod(*a, out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def prodT_kernel(nt, *a):
    out = np.zeros(6, dtype=np.int32)
    nt.nt_choose_prodT(*a, out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def cprod_kernel(nt, *a):
    out = np.zeros(8, dtype=np.int32)
    nt.nt_choose_cprod(np.array(a, dtype=np.int32).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def T(*rec):   # k_prodT<NB, hasq, 2, 16, tag, sgb, naskip, sparse>
    return ("k_prodT",) + rec


def P(*rec):   # k_prod<NB, contig, rawp, hasq, tag, tiled>
    return ("k_prod",) + rec


BYTE = ("k_prod8",)

# name, facts -> (refuse, smaj, vmax, m_pad, wgx, ky, smaj_cps, mc, sparse_ok), the kernel of the first launch (no warm start, the
# host rule has not chosen the skipping kernels, the tiled copy exists).  A refusal pins `refuse` alone.
# 400 000 x 1 000 000 on 256 CUs: 18 slabs of 109 chunks for two and for three column blocks (a comment in prod_planes said 17).
PLAN_TABLE = [
    ("full 16x3", dict(bits=2, n=400000, m=1000000, pitch=100096, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=3, ncu=256, segmented=0),
     (0, 1, 16, 1000448, 782, 18, 109, 55616, 1), T(3, 1, 0, 3, 0, 1)),
    ("full 16x2", dict(bits=2, n=400000, m=1000000, pitch=100096, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=256, segmented=0),
     (0, 1, 16, 1000448, 782, 18, 109, 55616, 1), T(2, 1, 0, 3, 0, 0)),
    ("full 16x2 304cu", dict(bits=2, n=400000, m=1000000, pitch=100096, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=304, segmented=0),
     (0, 1, 16, 1000448, 782, 12, 163, 83392, 1), T(2, 1, 0, 3, 0, 0)),
    ("full 16x3 304cu", dict(bits=2, n=400000, m=1000000, pitch=100096, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=3, ncu=304, segmented=0),
     (0, 1, 16, 1000448, 782, 12, 163, 83392, 1), T(3, 1, 0, 3, 0, 1)),
    ("full 8x2 no copy", dict(bits=2, n=400000, m=1000000, pitch=100096, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=8, S=2, ncu=256, segmented=0),
     (0, 0, 16, 1000000, 391, 9, 0, 111168, 0), P(1, 1, 1, 1, 0, 1)),
    ("shard 16x3", dict(bits=2, n=400000, m=125000, pitch=100096, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=3, ncu=256, segmented=0),
     (0, 1, 16, 125440, 782, 9, 28, 13952, 1), T(3, 1, 0, 3, 0, 1)),
    ("shard 16x2", dict(bits=2, n=400000, m=125000, pitch=100096, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=256, segmented=0),
     (0, 1, 16, 125440, 782, 11, 23, 11456, 1), T(2, 1, 0, 3, 0, 0)),
    ("shard 16x2 no copy", dict(bits=2, n=400000, m=125000, pitch=100096, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=256, segmented=0),
     (0, 0, 16, 125056, 391, 11, 0, 11392, 0), P(2, 1, 1, 1, 0, 1)),
    ("c2 8x2", dict(bits=2, n=50000, m=200000, pitch=12544, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=8, S=2, ncu=256, segmented=0),
     (0, 0, 16, 200000, 49, 10, 0, 20032, 0), P(1, 1, 1, 1, 0, 1)),
    ("3001x5003 16x3 copy", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=3, ncu=256, segmented=0),
     (0, 1, 16, 5120, 6, 5, 2, 1024, 1), T(3, 1, 0, 3, 0, 1)),
    ("3001x5003 16x2 copy", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=256, segmented=0),
     (0, 1, 16, 5120, 6, 5, 2, 1024, 1), T(2, 1, 0, 3, 0, 0)),
    ("3001x5003 8x2 copy", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=8, S=2, ncu=256, segmented=0),
     (0, 0, 16, 5056, 3, 1, 0, 5056, 0), P(1, 1, 1, 1, 0, 1)),
    ("3001x5003 16x3", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=3, ncu=256, segmented=0),
     (0, 0, 10, 5056, 3, 40, 0, 128, 0), P(2, 1, 1, 1, 0, 1)),
    ("3001x5003 16x2", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=256, segmented=0),
     (0, 0, 16, 5056, 3, 40, 0, 128, 0), P(2, 1, 1, 1, 0, 1)),
    ("3001x5003 8x2", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=8, S=2, ncu=256, segmented=0),
     (0, 0, 16, 5056, 3, 1, 0, 5056, 0), P(1, 1, 1, 1, 0, 1)),
    ("3001x5003 16x3 complete", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=0, no_sparse=0, nvec=16, S=3, ncu=256, segmented=0),
     (0, 1, 16, 5120, 6, 5, 2, 1024, 0), T(3, 0, 0, 3, 0, 0)),
    ("3001x5003 16x3 no sparse", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=1, nvec=16, S=3, ncu=256, segmented=0),
     (0, 1, 16, 5120, 6, 5, 2, 1024, 0), T(3, 1, 0, 3, 0, 0)),
    ("3001x5003 16x2 scattered", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=0, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=256, segmented=0),
     (0, 0, 16, 5056, 3, 40, 0, 128, 0), P(2, 0, 1, 1, 0, 0)),
    ("640x270000 16x3", dict(bits=2, n=640, m=270000, pitch=256, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=3, ncu=256, segmented=0),
     (0, 1, 16, 270336, 2, 24, 22, 11264, 1), T(3, 1, 0, 3, 0, 1)),
    ("2500x4096 5x7", dict(bits=2, n=2500, m=4096, pitch=768, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=5, S=7, ncu=256, segmented=0),
     (0, 1, 6, 4096, 5, 4, 2, 1024, 0), T(3, 1, 0, 3, 0, 0)),
    ("col0=64 16x3", dict(bits=2, n=3001, m=4939, pitch=768, col0=64, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=3, ncu=256, segmented=0),
     (0, 0, 10, 4992, 3, 39, 0, 128, 0), P(2, 1, 1, 1, 0, 1)),
    ("col0=512 16x3", dict(bits=2, n=3001, m=4491, pitch=768, col0=512, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=3, ncu=256, segmented=0),
     (0, 1, 16, 4608, 6, 5, 2, 960, 1), T(3, 1, 0, 3, 0, 1)),
    ("byte 132352 m=132097", dict(bits=8, n=132352, m=132097, pitch=132352, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=8, S=2, ncu=256, segmented=0),
     (0, 0, 16, 132160, 517, 8, 0, 16576, 0), BYTE),
    ("byte 300x700", dict(bits=8, n=300, m=700, pitch=512, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=11, S=2, ncu=256, segmented=0),
     (0, 0, 16, 704, 2, 11, 0, 64, 0), BYTE),
    ("m_pad 2500032 8x2", dict(bits=2, n=3001, m=2500001, pitch=768, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=8, S=2, ncu=256, segmented=0),
     (0, 0, 16, 2500032, 3, 64, 0, 39104, 0), P(1, 1, 1, 1, 0, 1)),
    ("m_pad 2500096 16x2 copy", dict(bits=2, n=3001, m=2500001, pitch=768, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=256, segmented=0),
     (0, 1, 16, 2500096, 6, 24, 204, 104192, 1), T(2, 1, 0, 3, 0, 0)),
    ("row sums 1x7", dict(bits=2, n=3001, m=5003, pitch=768, col0=0, cols_contig=1, have_smaj=1, mode=2, raw_na=0, has_q=1, no_sparse=0, nvec=1, S=7, ncu=256, segmented=0),
     (0, 0, 4, 5056, 3, 1, 0, 5056, 0), P(1, 1, 0, 1, 0, 1)),
    ("segments no copy", dict(bits=2, n=400000, m=125000, pitch=100096, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=256, segmented=1),
     (2, 0, 1, 0, 0, 1, 0, 0, 0), None),
    ("segments copy", dict(bits=2, n=400000, m=125000, pitch=100096, col0=0, cols_contig=1, have_smaj=1, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=16, S=2, ncu=256, segmented=1),
     (0, 1, 16, 125440, 782, 11, 23, 11456, 1), T(2, 1, 0, 3, 0, 0)),
    ("pitch limit", dict(bits=2, n=68000000, m=1000, pitch=17000192, col0=0, cols_contig=1, have_smaj=0, mode=1, raw_na=1, has_q=1, no_sparse=0, nvec=8, S=2, ncu=256, segmented=0),
     (1, 0, 1, 0, 0, 1, 0, 0, 0), None),
]


@pytest.mark.parametrize("name,kw,want,kernel", PLAN_TABLE, ids=[r[0] for r in PLAN_TABLE])
def test_plan_prod(nt, name, kw, want, kernel):
    got = plan(nt, **kw)
    if want[0] != NONE:
        assert got[0] == want[0] and kernel is None
        return
    assert got == want
    refuse, smaj, vmax, m_pad, wgx, ky, cps, mc, sparse_ok = got
    # the slabs cover the variants, none beyond the int32 bound of its image
    if smaj:
        assert m_pad % 512 == 0 and ky * cps >= m_pad // 512 > (ky - 1) * cps and cps * 512 <= 2500000
    else:
        assert m_pad % 64 == 0 and mc % 64 == 0 and ky * mc >= m_pad > (ky - 1) * mc and mc <= (132096 if kw["bits"] == 8 else 2500000)
    NB = nt.nt_pick_nb(min(kw["nvec"], vmax) * kw["S"])
    if smaj and NB >= 2:
        got_k = T(*prodT_kernel(nt, NB, kw["has_q"], 0, 0, sparse_ok))
    elif kw["bits"] == 8:
        got_k = BYTE
    else:
        assert NB <= 2   # (k_prod has two column blocks at most)
        got_k = P(*prod_kernel(nt, NB, kw["cols_contig"], kw["cols_contig"] and kw["col0"] % 64 == 0, kw["raw_na"], kw["has_q"], 0))
    assert got_k == kernel


def test_named_points(nt):
    by = {r[0]: r for r in PLAN_TABLE}
    assert by["full 16x3"][2][5:7] == by["full 16x2"][2][5:7] == (18, 109)           # 782 x 18 workgroups = 54.98 rounds of 256
    assert by["c2 8x2"][2][5] == 10                                                   # the 4 % cap, then the best fill of 512
    assert by["2500x4096 5x7"][2][8] == 0 and by["2500x4096 5x7"][2][1] == 1          # 56-bit panel: k_prodT, dense
    assert by["col0=64 16x3"][2][1:3] == (0, 10)                                      # no k_prodT: 16 x 3 goes as two launches of k_prod
    assert by["byte 132352 m=132097"][2][7] <= 132096 < by["byte 132352 m=132097"][2][3]
    assert by["m_pad 2500096 16x2 copy"][2][6] * 512 <= 2500000 < by["m_pad 2500096 16x2 copy"][2][3]
    assert by["m_pad 2500032 8x2"][2][7] <= 2500000 < by["m_pad 2500032 8x2"][2][3]
    assert by["segments no copy"][2][0] == NOTHING_QUEUED and by["pitch limit"][2][0] == PITCH_LIMIT


def test_slab_override(nt):
    """the slab sweeps of the profiling build (BSN_KY, BSN_KY_T): one override each, clamped like the rule's own choice"""
    shard = dict(PLAN_TABLE[6][1])
    assert plan(nt, **shard)[5:7] == (11, 23)
    assert plan(nt, ky_t=8, **shard)[5:7] == (8, 31)
    assert plan(nt, ky_t=1000, **shard)[5:7] == (245, 1)          # at most one slab per chunk
    assert plan(nt, ky=8, **shard)[5:7] == (11, 23)               # BSN_KY is k_prod's
    plain = dict(PLAN_TABLE[7][1])
    assert plan(nt, **plain)[5] == 11 and plan(nt, ky_t=5, **plain)[5] == 11
    assert plan(nt, ky=5, **plain)[5] == 5 and plan(nt, ky=100000, **plain)[5] == 1954   # at most one slab per 64-variant step


def test_vectors_per_launch(nt):
    lim = np.zeros(2, dtype=np.int32)
    nt.nt_prod_limits(lim.ctypes.data_as(C.c_void_p))
    assert tuple(lim) == (48, 32)
    assert [nt.nt_pick_nb(c) for c in (1, 16, 17, 32, 33, 48)] == [1, 1, 2, 2, 3, 3]
    # three column blocks on a 2-bit image unless the launch also counts the codes
    assert [nt.nt_cprod_vmax(2, 0, S) for S in range(1, 9)] == [32, 24, 16, 12, 9, 8, 6, 6]
    assert [nt.nt_cprod_vmax(2, 1, S) for S in range(1, 9)] == [32, 16, 10, 8, 6, 5, 4, 4]
    assert [nt.nt_cprod_vmax(8, 0, S) for S in range(1, 9)] == [32, 16, 10, 8, 6, 5, 4, 4]


# (NB, plain, stats, cols_contig, tiled, warm, na_skip) -> k_cprod<NB, ., 512, ., ., contig, tiles, waves, 1, tag, tiled, sgb, naskip>
CPROD_TABLE = [
    ((1, 1, 0, 1, 0, 0, 0), (1, 1, 2, 8, 0, 0, 0, 0)),
    ((1, 1, 0, 1, 0, 1, 0), (1, 1, 2, 8, 1, 0, 0, 0)),     # warm start: its own name
    ((1, 1, 0, 0, 0, 0, 0), (1, 0, 2, 8, 0, 0, 0, 0)),
    ((1, 1, 0, 0, 0, 1, 0), (1, 0, 2, 8, 0, 0, 0, 0)),     # ... which gathered variants do not have
    ((1, 1, 0, 1, 1, 0, 0), (1, 1, 4, 8, 0, 1, 0, 0)),     # tiled copy: 4 tiles per wave
    ((1, 1, 0, 1, 1, 1, 0), (1, 1, 4, 8, 1, 1, 0, 0)),
    ((1, 0, 1, 1, 1, 0, 0), (1, 1, 2, 8, 0, 1, 0, 0)),     # the counting pass keeps 2
    ((1, 0, 0, 1, 1, 0, 0), (1, 1, 4, 8, 0, 1, 0, 0)),     # one- and three-plane passes
    ((2, 0, 1, 1, 1, 0, 0), (2, 1, 2, 16, 0, 1, 3, 0)),
    ((2, 1, 0, 1, 0, 0, 0), (2, 1, 2, 16, 0, 0, 3, 0)),
    ((2, 1, 0, 0, 0, 0, 0), (2, 0, 2, 16, 0, 0, 0, 0)),
    ((2, 1, 0, 1, 1, 1, 0), (2, 1, 2, 16, 0, 1, 3, 0)),    # two blocks: no warm-start name
    ((3, 1, 0, 1, 1, 0, 0), (3, 1, 2, 16, 0, 0, 3, 0)),    # three blocks: the plain image, whether or not the tiled copy serves
    ((3, 1, 0, 0, 0, 0, 0), (3, 0, 2, 16, 0, 0, 0, 0)),
    ((3, 0, 0, 1, 0, 0, 1), (3, 1, 2, 16, 0, 0, 3, 0)),    # complete data: no plane to skip
    ((2, 1, 0, 1, 1, 0, 1), (2, 1, 2, 16, 0, 0, 0, 1)),    # skipping kernels: plain image, no explicit schedule
    ((2, 1, 0, 0, 0, 0, 1), (2, 0, 2, 16, 0, 0, 0, 1)),
    ((3, 1, 0, 1, 0, 0, 1), (3, 1, 2, 16, 0, 0, 0, 1)),
    ((3, 1, 0, 0, 0, 0, 1), (3, 0, 2, 16, 0, 0, 0, 1)),
    ((1, 1, 0, 1, 1, 0, 1), (1, 1, 4, 8, 0, 1, 0, 0)),     # one block has none
    ((2, 0, 1, 1, 0, 0, 1), (2, 1, 2, 16, 0, 0, 3, 0)),    # nor has the counting pass
]
# (NB, has_q, warm, na_skip, sparse_ok) -> k_prodT<NB, hasq, 2, 16, tag, sgb, naskip, sparse>
PRODT_TABLE = [
    ((3, 1, 0, 0, 1), (3, 1, 0, 3, 0, 1)),
    ((3, 1, 1, 0, 1), (3, 1, 1, 3, 0, 1)),
    ((3, 1, 0, 1, 1), (3, 1, 0, 0, 1, 0)),                 # the skipping kernels come before the sparse form
    ((3, 1, 0, 0, 0), (3, 1, 0, 3, 0, 0)),
    ((3, 1, 1, 0, 0), (3, 1, 0, 3, 0, 0)),                 # dense k_prodT<3> has no warm-start name
    ((3, 0, 0, 0, 0), (3, 0, 0, 3, 0, 0)),
    ((3, 0, 1, 1, 0), (3, 0, 0, 3, 0, 0)),
    ((2, 1, 0, 0, 1), (2, 1, 0, 3, 0, 0)),                 # sparse only with three column blocks
    ((2, 1, 1, 0, 1), (2, 1, 1, 3, 0, 0)),
    ((2, 1, 1, 1, 1), (2, 1, 0, 0, 1, 0)),
    ((2, 0, 1, 1, 0), (2, 0, 1, 3, 0, 0)),
    ((2, 0, 0, 0, 0), (2, 0, 0, 3, 0, 0)),
]
# (NB, cols_contig, tiled, rawp, has_q, warm) -> k_prod<NB, contig, rawp, hasq, tag, tiled>
PROD_TABLE = [
    ((1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 0, 1)),
    ((1, 1, 1, 1, 1, 1), (1, 1, 1, 1, 1, 1)),
    ((2, 1, 0, 1, 0, 1), (2, 1, 1, 0, 1, 0)),
    ((1, 0, 0, 1, 1, 1), (1, 0, 1, 1, 1, 0)),
    ((1, 1, 1, 0, 1, 1), (1, 1, 0, 1, 0, 1)),              # a look-up plane has no warm-start name
    ((1, 1, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0)),
    ((2, 0, 0, 1, 1, 0), (2, 0, 1, 1, 0, 0)),
]


@pytest.mark.parametrize("facts,want", CPROD_TABLE)
def test_choose_cprod(nt, facts, want):
    assert cprod_kernel(nt, *facts) == want


@pytest.mark.parametrize("facts,want", PRODT_TABLE)
def test_choose_prodT(nt, facts, want):
    assert prodT_kernel(nt, *facts) == want


@pytest.mark.parametrize("facts,want", PROD_TABLE)
def test_choose_prod(nt, facts, want):
    assert prod_kernel(nt, *facts) == want


def test_every_k_prodT_instance_is_in_the_table(nt):
    assert len({w for _, w in PRODT_TABLE}) == 10   # the ten instances launch_prodT lists
