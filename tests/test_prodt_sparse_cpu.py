"""k_prodT's sparse form without a GPU: the decode of bigsnpr_amd/csrc/prodt_sparse.hpp (the header the kernel compiles),
built with g++ — every field of a genotype dword gives the compressed value {0, 1, 2, 1} for the codes {0, 1, 2, 3} and
the index 2 (f & 1) + missing, a group's two indices distinct and ascending —, and the statement "compressed values +
index x interleaved digits" against the two-plane sum code . A + missing . (B - 3 A) the dense kernels add."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import prodt_sparse_ref as ref  # noqa: E402

VALUE = np.array([0, 1, 2, 1])


def check_decode(w):
    w = np.asarray(w, dtype=np.uint32)
    vals, fields = ref.decode(w)
    codes = (w[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3
    np.testing.assert_array_equal(vals, VALUE[codes])
    np.testing.assert_array_equal(fields, 2 * (np.arange(16) & 1)[None, :] + (codes == 3))
    assert np.all(fields[:, 0::2] < fields[:, 1::2])          # distinct and ascending in every group


def test_every_byte_value_in_every_byte_position():
    for pos in range(4):
        check_decode(np.arange(256, dtype=np.uint32) << np.uint32(8 * pos))
        # ... and beside neighbours that are all 2 / all missing (a carry or a borrow between fields would show)
        for fill in (0xAAAAAAAA, 0xFFFFFFFF, 0x55555555):
            keep = np.uint32(fill & ~(0xFF << (8 * pos)) & 0xFFFFFFFF)
            check_decode((np.arange(256, dtype=np.uint32) << np.uint32(8 * pos)) | keep)


def test_random_dwords():
    rng = np.random.default_rng(5)
    check_decode(rng.integers(0, 2 ** 32, 10000, dtype=np.uint64).astype(np.uint32))


def two_plane(w, dA, dB):
    """what the dense kernels add for the 16 variants of w: code (3 for missing) x A digits + missing x (B - 3 A) —
    with exact integers A, B in place of their digits, so that B - 3 A needs no digit of its own"""
    codes = (int(w) >> (2 * np.arange(16))) & 3
    return int(np.sum(codes * dA.astype(np.int64) + (codes == 3) * (dB.astype(np.int64) - 3 * dA.astype(np.int64))))


def test_values_and_index_times_interleaved_digits():
    rng = np.random.default_rng(9)
    pat = []
    for q in range(8):                                         # the four combinations in every pair position
        for c0 in (rng.integers(0, 3), 3):
            for c1 in (rng.integers(0, 3), 3):
                w = int(rng.integers(0, 2 ** 32)) & ~(0xF << (4 * q)) | (int(c0) << (4 * q)) | (int(c1) << (4 * q + 2))
                pat.append(w)
    pat += [0xFFFFFFFF, 0, 0xAAAAAAAA, 0x55555555, 0xEEEEEEEE, 0xBBBBBBBB]     # all missing / none / all 2 / all 1 / (2, 3) / (3, 2)
    pat += [int(x) for x in rng.integers(0, 2 ** 32, 2000)]
    for i, w in enumerate(pat):
        if i % 3 == 0:                                         # digits at the ends of int8
            dA, dB = rng.choice([-128, 127], 16).astype(np.int8), rng.choice([-128, 127], 16).astype(np.int8)
        else:
            dA, dB = rng.integers(-128, 128, 16).astype(np.int8), rng.integers(-128, 128, 16).astype(np.int8)
        s, legal = ref.dot(w, dA, dB)
        assert legal, hex(w)
        assert s == two_plane(w, dA, dB), hex(w)
