"""The kernel choice of the windowed-LD band (bigsnpr_amd/csrc/ld_plan.hpp: plan_band, xy_kernel, small_band_kernel,
k_split) and the split geometry of the byte image (byte_xy_split, byte_na_split, byte_plan.hpp), pinned on the CPU through
tests/native.  The expected values are literal: they were written from the
conditions of band_run as it stood before the decision was moved out of it, one row per kernel id that
bsn_ld_last_stats can report (0-4, 6-11) and one on either side of every threshold."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

BYTE_NA, BYTE_XY, SHARED, XY, SMALL = range(5)     # LdPath
COR, R2, CLUMP_FBM, CLUMP_BED = range(4)           # LdMode
FIELDS = ("bits", "pitch", "n", "mode", "complete", "contig", "all_rows", "have_cnn", "npairs_b", "i8", "lut", "no_quad")
# a 2-bit image of 4 000 samples (1 024 bytes per variant), all of them selected, missing values, a contiguous ind.col
# and a band of 2 000 blocks: the raw-plane kernel
BASE = dict(bits=2, pitch=1024, n=4000, mode=COR, complete=0, contig=1, all_rows=1, have_cnn=1, npairs_b=2000,
            i8=0, lut=0, no_quad=0)


@pytest.fixture(scope="module")
def nt():
    import build_native
    lib = C.CDLL(build_native.build())
    lib.nt_ld_xy_kernel.argtypes = [C.c_void_p, C.c_int64]
    lib.nt_ld_k_split.argtypes = [C.c_int64] * 4 + [C.c_void_p]
    lib.nt_byte_xy_split.argtypes = lib.nt_byte_na_split.argtypes = [C.c_int64] * 2 + [C.c_void_p]
    lib.nt_byte_limits.argtypes = [C.c_void_p]
    lib.nt_byte_min_slabs.argtypes = [C.c_int64]
    lib.nt_slab_variants.argtypes = [C.c_int64] * 2
    lib.nt_byte_min_slabs.restype = lib.nt_slab_variants.restype = C.c_int64
    return lib


def facts(**kw):
    assert set(kw) <= set(FIELDS)
    f = dict(BASE, **kw)
    return np.array([f[k] for k in FIELDS], dtype=np.int64)


def plan(nt, **kw):
    out = np.zeros(6, dtype=np.int32)
    nt.nt_ld_plan(facts(**kw).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


# (facts that differ from BASE) -> (path, kernel id, f4, raw, nomask, quad_all)
PLAN_TABLE = [
    # --- six / four sums with enough blocks: the column operand decoded once per workgroup
    (dict(), (SHARED, 10, 1, 1, 1, 0)),
    (dict(mode=R2), (SHARED, 10, 1, 1, 1, 0)),
    (dict(mode=CLUMP_BED), (SHARED, 11, 1, 1, 1, 0)),
    (dict(all_rows=0), (SHARED, 10, 1, 1, 0, 0)),
    (dict(mode=CLUMP_BED, all_rows=0), (SHARED, 11, 1, 1, 0, 0)),
    (dict(lut=1), (SHARED, 6, 1, 0, 0, 0)),                       # BSN_LD_LUT: the look-up planes, always with the mask
    (dict(lut=1, mode=CLUMP_BED), (SHARED, 9, 1, 0, 0, 0)),
    (dict(have_cnn=0), (SHARED, 6, 1, 0, 0, 0)),                  # no per-variant counts on the device: no raw planes
    (dict(i8=1), (SHARED, 4, 0, 0, 0, 0)),                        # BSN_LD_I8
    (dict(i8=1, mode=CLUMP_BED), (SHARED, 4, 0, 0, 0, 0)),
    (dict(i8=1, lut=1), (SHARED, 4, 0, 0, 0, 0)),
    (dict(no_quad=1), (SHARED, 10, 1, 1, 1, 0)),                  # BSN_LD_NO_QUAD belongs to the cross-product path
    # 9 n < 2^24 for the raw planes: 4 pitch <= 1 864 135
    (dict(pitch=466033, n=1864000), (SHARED, 10, 1, 1, 1, 0)),    # 4 pitch = 1 864 132
    (dict(pitch=466034, n=1864000), (SHARED, 6, 1, 0, 0, 0)),     # 4 pitch = 1 864 136
    (dict(pitch=466034, n=1864000, mode=CLUMP_BED), (SHARED, 9, 1, 0, 0, 0)),
    # 4 n < 2^24 for the FP4 pipe: 4 pitch <= 4 194 303
    (dict(pitch=1048575, n=4194000), (SHARED, 6, 1, 0, 0, 0)),    # 4 pitch = 4 194 300
    (dict(pitch=1048576, n=4194000), (SHARED, 4, 0, 0, 0, 0)),    # 4 pitch = 4 194 304
    # --- too few blocks, or a scattered ind.col: 64 x 64 tile pairs, K split decided per batch
    (dict(npairs_b=1024), (SHARED, 10, 1, 1, 1, 0)),
    (dict(npairs_b=1023), (SMALL, 1, 0, 0, 0, 0)),
    (dict(contig=0), (SMALL, 1, 0, 0, 0, 0)),
    (dict(contig=0, mode=CLUMP_BED, i8=1, lut=1), (SMALL, 1, 0, 0, 0, 0)),
    # --- cross product only: no missing value among the selected samples, or the FBM clumping formula
    (dict(complete=1), (XY, 7, 1, 0, 1, 1)),
    (dict(complete=1, mode=R2), (XY, 7, 1, 0, 1, 1)),
    (dict(complete=1, mode=CLUMP_BED), (XY, 7, 1, 0, 1, 1)),
    (dict(mode=CLUMP_FBM), (XY, 7, 1, 0, 1, 1)),                  # with missing values too (src/clumping.cpp:66-73)
    (dict(complete=1, all_rows=0), (XY, 7, 1, 0, 0, 1)),
    (dict(complete=1, no_quad=1), (XY, 7, 1, 0, 1, 0)),
    (dict(complete=1, i8=1), (XY, 2, 0, 0, 0, 0)),
    (dict(complete=1, lut=1), (XY, 7, 1, 0, 1, 1)),               # BSN_LD_LUT belongs to the six-sum path
    (dict(complete=1, contig=0, npairs_b=3), (XY, 7, 1, 0, 1, 1)),
    # here the limit is on the samples of the image, not on its pitch
    (dict(complete=1, pitch=1048576, n=4194303), (XY, 7, 1, 0, 1, 1)),
    (dict(complete=1, pitch=1048576, n=4194304), (XY, 2, 0, 0, 0, 0)),
    # --- byte image (dosage grid): nothing but missingness and the formula decides
    (dict(bits=8), (BYTE_NA, 3, 0, 0, 0, 0)),
    (dict(bits=8, mode=R2), (BYTE_NA, 3, 0, 0, 0, 0)),
    (dict(bits=8, i8=1, lut=1, no_quad=1, contig=0), (BYTE_NA, 3, 0, 0, 0, 0)),
    (dict(bits=8, complete=1), (BYTE_XY, 2, 0, 0, 0, 0)),
    (dict(bits=8, mode=CLUMP_FBM), (BYTE_XY, 2, 0, 0, 0, 0)),     # its NaN for a missing dosage is k_band_fill8's
    (dict(bits=8, complete=1, mode=CLUMP_FBM, npairs_b=5), (BYTE_XY, 2, 0, 0, 0, 0)),
]


@pytest.mark.parametrize("kw,want", PLAN_TABLE, ids=[",".join("%s=%s" % kv for kv in kw.items()) or "base" for kw, _ in PLAN_TABLE])
def test_plan_band(nt, kw, want):
    assert plan(nt, **kw) == want


def test_every_kernel_id_is_in_the_table(nt):
    per_batch = {0, 1, 8}   # decided per batch: below
    assert {w[1] for _, w in PLAN_TABLE} | per_batch == {0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11}


def test_per_batch_choices(nt):
    def xy(np_, **kw):
        return nt.nt_ld_xy_kernel(facts(complete=1, **kw).ctypes.data_as(C.c_void_p), np_)
    # 2 x 2 blocks of tile pairs once a batch has 64 of them
    assert xy(63) == 7 and xy(64) == 8 and xy(4096) == 8
    assert xy(64, no_quad=1) == 7
    assert xy(64, i8=1) == 2 and xy(63, i8=1) == 2
    assert xy(64, all_rows=0) == 8
    # the fused epilogue needs the whole sample range in one workgroup
    assert nt.nt_ld_small_band_kernel(1) == 0
    assert nt.nt_ld_small_band_kernel(2) == 1 and nt.nt_ld_small_band_kernel(8) == 1


# k_split(pitch, want, align, min_bytes) -> (splits, bytes per split):
#   s = max(1, min(want, pitch // min_bytes)); bytes = round_up(ceil(pitch / s), align); splits = ceil(pitch / bytes)
K_SPLIT_TABLE = [
    # six sums, 100 tile pairs: want = max(1, 2048 // 100) = 20; min(20, 1024 // 256 = 4) = 4; ceil(1024 / 4) = 256 -> 256; 1024 / 256 = 4
    ((1024, 20, 64, 256), (4, 256)),
    # six sums, a full batch of 4 096: want = max(1, 2048 // 4096 = 0) = 1; one split of round_up(1024, 64) = 1024: the fused kernel
    ((1024, 1, 64, 256), (1, 1024)),
    # cross product, 300 pairs: want = max(4, 8192 // 300 = 27) = 27; min(27, 1280 // 256 = 5) = 5; 1280 / 5 = 256 -> 256; 5 splits
    ((1280, 27, 128, 256), (5, 256)),
    # cross product, 4 096 pairs: want = max(4, 2) = 4; min(4, 1088 // 256 = 4) = 4; ceil(1088 / 4) = 272 -> 384 (whole cache
    # lines); ceil(1088 / 384) = 3: rounding up the split can lower the count
    ((1088, 4, 128, 256), (3, 384)),
    # 2 x 2 blocks, 1 024 of them: want = max(1, 4096 // 1024) = 4; min(4, 4096 // 1024 = 4) = 4; 4096 / 4 = 1024 -> 1024; 4 splits
    ((4096, 4, 128, 1024), (4, 1024)),
    # a row shorter than min_bytes: 64 // 256 = 0 -> 1 split of round_up(64, 64) = 64
    ((64, 20, 64, 256), (1, 64)),
    # byte image of one slice, 2 pairs: want = 8192 // 2 = 4096; min(4096, 100032 // 256 = 390) = 390;
    # ceil(100032 / 390) = 257 -> 320; ceil(100032 / 320) = 313 (312 x 320 = 99 840 < 100 032)
    ((100032, 4096, 64, 256), (313, 320)),
]


@pytest.mark.parametrize("args,want", K_SPLIT_TABLE)
def test_k_split(nt, args, want):
    out = np.zeros(2, dtype=np.int64)
    nt.nt_ld_k_split(*args, out.ctypes.data_as(C.c_void_p))
    assert (int(out[0]), int(out[1])) == want
    assert out[0] * out[1] >= args[0] and out[1] % args[2] == 0   # the splits cover the row in aligned pieces


# ---- byte image: the exact-integer size argument (byte_plan.hpp) and the two split rules band_run launches with -----------------
SLICE = 131072
# every slice count, ragged and exact multiples, and the neighbours of a boundary (a pitch is a multiple of 256)
BYTE_PITCHES = sorted({256, 512, 1280, 100096, SLICE - 256, SLICE, SLICE + 256, 135424, 2 * SLICE - 256, 2 * SLICE, 2 * SLICE + 256,
                       3 * SLICE - 4096, 3 * SLICE, 3 * SLICE + 256, 4 * SLICE, 4 * SLICE + 65536, 5 * SLICE, 5 * SLICE + 256, 6 * SLICE - 256,
                       6 * SLICE} | {s * SLICE + 256 * 37 * s for s in range(1, 6)})
BYTE_NP = sorted(set(range(1, 40)) | {2 ** e for e in range(13)} | {2 ** e + 1 for e in range(12)} | {2 ** e - 1 for e in range(2, 13)} |
                 {100, 300, 511, 513, 1000, 3000})


def _limits(nt):
    out = np.zeros(4, dtype=np.int64)
    nt.nt_byte_limits(out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def test_byte_limits(nt):
    slice_bytes, max_slices, term_max, slab = _limits(nt)
    assert (slice_bytes, max_slices, term_max) == (SLICE, 6, 127 * 128)
    assert term_max * slice_bytes < 2 ** 31                       # one slice of samples fits an int32 accumulator
    assert slab % 64 == 0 and slab <= (2 ** 31 - 1) // term_max == 132104 < slab + 64   # and so does one slab of variants
    assert BYTE_PITCHES[0] == 256 and BYTE_PITCHES[-1] == max_slices * slice_bytes and BYTE_NP[0] == 1 and BYTE_NP[-1] == 4096
    assert {-(-p // SLICE) for p in BYTE_PITCHES} == {1, 2, 3, 4, 5, 6}
    assert all(any(-(-p // SLICE) == s and p % SLICE != 0 for p in BYTE_PITCHES) for s in range(1, 7))


@pytest.mark.parametrize("pitch", BYTE_PITCHES)
def test_byte_xy_split(nt, pitch):
    """k_pair_xy8: grid y = splits per slice x slices, split y covers [y bytes, (y + 1) bytes) and adds to plane y // splits"""
    out = np.zeros(3, dtype=np.int64)
    for np_ in BYTE_NP:
        nt.nt_byte_xy_split(pitch, np_, out.ctypes.data_as(C.c_void_p))
        nslice, splits, nbytes = (int(v) for v in out)
        assert nslice == -(-pitch // SLICE) and splits >= 1
        grid_y = splits * nslice
        assert nbytes % 64 == 0 and nbytes >= 64
        assert grid_y * nbytes >= pitch                            # the splits cover [0, pitch)
        b0 = np.arange(grid_y, dtype=np.int64) * nbytes
        b1 = np.minimum(b0 + nbytes, pitch)
        live = b0 < b1
        assert live[0] and b1[live][-1] == pitch and np.all(b0[live][1:] == b1[live][:-1])
        plane = np.arange(grid_y) // splits                        # the kernel's `slice`
        assert np.all(b0[live] // SLICE == plane[live]) and np.all((b1[live] - 1) // SLICE == plane[live])   # none straddles
        assert plane.max() == nslice - 1
        if nslice == 1:                                            # one slice: k_split as before
            k = np.zeros(2, dtype=np.int64)
            nt.nt_ld_k_split(pitch, max(1, 8192 // np_), 64, 256, k.ctypes.data_as(C.c_void_p))
            assert (splits, nbytes) == (int(k[0]), int(k[1]))
        else:
            assert splits & (splits - 1) == 0 and splits * nbytes == SLICE and nbytes >= 256


@pytest.mark.parametrize("pitch", BYTE_PITCHES)
def test_byte_na_split(nt, pitch):
    """k_pair_stats8: grid y = splits over the whole row; a split adds int32 sums into int64 statistics, so only its length counts"""
    out = np.zeros(3, dtype=np.int64)
    for np_ in BYTE_NP:
        nt.nt_byte_na_split(pitch, np_, out.ctypes.data_as(C.c_void_p))
        nslice, splits, nbytes = (int(v) for v in out)
        assert nbytes % 64 == 0 and 64 <= nbytes <= SLICE          # no longer than a slice
        assert splits >= nslice and splits * nbytes >= pitch > (splits - 1) * nbytes   # cover [0, pitch), no empty split
        assert splits <= 65535


def test_byte_slabs(nt):
    """k_prod8: whatever number of slabs the grid rule of prod_planes asks for, none holds more than 132 104 variants"""
    slab = _limits(nt)[3]
    for m_pad in [64, 128, slab - 64, slab, slab + 64, 2 * slab, 2 * slab + 64, 1000000 // 64 * 64, 2500032, 5000000 // 64 * 64,
                  20 * slab + 64]:
        ky_min = nt.nt_byte_min_slabs(m_pad)
        assert ky_min == -(-m_pad // slab)
        assert ky_min == 1 or nt.nt_slab_variants(m_pad // 64, ky_min - 1) > slab      # the bound is tight
        for ky in sorted({ky_min, ky_min + 1, 2 * ky_min, max(ky_min, 17), max(ky_min, 64)}):
            mc = nt.nt_slab_variants(m_pad // 64, ky)
            assert mc % 64 == 0 and 64 <= mc <= slab <= 132104 and mc * ky >= m_pad
