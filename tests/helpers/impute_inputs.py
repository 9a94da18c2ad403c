"""What the device tests of snp_fastImputeSimple share (tests/test_gpu_impute.py, tests/test_gpu_impute_shapes.py): the checks
of a result against the CPU statement (tests/native/impute_ref.py), and seeded inputs sized so that each loop of the kernels
of bigsnpr_amd/csrc/impute.hip takes a second turn.  The thresholds are read from the source (`kernel_constants`); the launch
geometry is restated here in Python (`rewrite_grid`, the pitches, the loop conditions), and tests/test_impute_shapes_cpu.py
proves without a GPU that each shape of `shapes` crosses the loop it is named for."""
import os
import re
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))

import impute_ref as ref  # noqa: E402

IMPUTE_HIP = os.path.join(ROOT, "bigsnpr_amd", "csrc", "impute.hip")
INTERNAL_HPP = os.path.join(ROOT, "bigsnpr_amd", "csrc", "bsn_internal.hpp")

METHODS = ("zero", "mode", "mean0", "mean2", "random")
SEED = ref.SEED


# ---- the checks of the device tests ---------------------------------------------------------------------------------------

def impute(ba, Gna, method, **kw):
    """snp_fastImputeSimple with its expected warnings let through"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ba.snp_fastImputeSimple(Gna, method, **kw)


def column(ba, res, j):
    """decoded column j of a result, through the accessor (2-bit image; -1 = missing) or a product with e_j (byte image;
    in hundredths)"""
    if res.bits == 2:
        return ba.read_bed(res._bed, np.arange(res.nrow), np.array([j]))[:, 0]
    e = np.zeros(res.ncol)
    e[j] = 1.0
    return np.rint(100 * ba.big_prodVec(res, e)).astype(np.int64)


def same_image(ba, res, n_vec_seed=3):
    """`res` against a second FBM_code256 uploaded from its bytes under its table"""
    twin = ba.FBM_code256(res.bytes, res.code256)
    assert twin.bits == res.bits and twin._has_na == res._has_na
    a, b = ba.snp_colstats(res), ba.snp_colstats(twin)
    np.testing.assert_array_equal(a["sumX"], b["sumX"])
    np.testing.assert_array_equal(a["denoX"], b["denoX"])
    if res.bits == 2:
        np.testing.assert_array_equal(res._bed.download(), twin._bed.download())   # pad bits included
    if not res._has_na:
        rng = np.random.default_rng(n_vec_seed)
        x, y = rng.integers(-3, 4, res.ncol).astype(np.float64), rng.integers(-3, 4, res.nrow).astype(np.float64)
        np.testing.assert_array_equal(ba.big_prodVec(res, x), ba.big_prodVec(twin, x))
        np.testing.assert_array_equal(ba.big_cprodVec(res, y), ba.big_cprodVec(twin, y))
    return twin


def edge_matrix(n, m):
    """random calls with a third missing; for m = 65: variant 1 complete, 2 all missing, 3 / 4 with their only missing call
    at the first / last sample, 64 (the last) all missing too; for m = 1 the caller passes the kind"""
    rng = np.random.default_rng(1000 * n + m)
    g = rng.integers(0, 3, (n, m)).astype(np.uint8)
    g[rng.random((n, m)) < 0.33] = 3
    if m > 4:
        g[:, 1] = rng.integers(0, 3, n)
        g[:, 2] = 3
        g[:, 3] = rng.integers(0, 3, n)
        g[0, 3] = 3
        g[:, 4] = rng.integers(0, 3, n)
        g[n - 1, 4] = 3
        g[:, m - 1] = 3
    return np.asfortranarray(g)


def check_edges(ba, g, method):
    want, _, want_all = ref.impute(g, method, seed=SEED)
    res = impute(ba, ba.FBM_code256(g), method, seed=SEED, return_bytes=True)
    assert np.array_equal(res.bytes, want)
    assert res.n_all_missing == want_all == int((g == 3).all(0).sum())
    stays = method in ("mean0", "mean2", "random") and want_all > 0
    assert res._has_na == stays
    allna = (g == 3).all(0)
    assert (res.bytes[:, allna] == (4 if method == "mode" else 3)).all()
    same_image(ba, res)
    if res.bits == 2:   # the all-missing variants through the accessor: 0 for zero / mode, still missing otherwise
        for j in np.flatnonzero(allna):
            assert (column(ba, res, j) == (-1 if stays else 0)).all()


# ---- the thresholds, from the source ----------------------------------------------------------------------------------------

CONSTANTS = ("kRewriteVecs", "kRewriteGroups", "kBytesMaxCols", "kBytesChunkMiB", "kBytesGroups", "kPitchAlign")

# fixed by the kernels' own index arithmetic (impute.hip): lanes of a wave, waves (= variants) of a workgroup, bytes of a
# vector, vectors a lane of k_impute_2bit takes per turn, threads of a workgroup of k_impute_bytes
WAVE, WAVES, VEC, PER_TURN, BYTES_THREADS = 64, 4, 16, 2, 256


def _constexpr(path, name):
    with open(path) as f:
        found = re.findall(r"^\s*constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, f.read(), flags=re.M)
    assert len(found) == 1, "%s: %d constexpr lines in %s" % (name, len(found), path)
    return int(found[0])


def kernel_constants():
    """the `constexpr` integers that decide when a loop of impute.hip's kernels goes round again"""
    return {name: _constexpr(INTERNAL_HPP if name == "kPitchAlign" else IMPUTE_HIP, name) for name in CONSTANTS}


def round_up(x, a):
    return (x + a - 1) // a * a


def pitch2(n, K):
    """bytes of a variant's row in the 2-bit image"""
    return round_up((n + 3) // 4, K["kPitchAlign"])


def pitch8(n, K):
    """bytes of a variant's row in the int8 image of `mean2`"""
    return round_up(n, K["kPitchAlign"])


def rewrite_grid(nvec, m, K):
    """impute.hip's rewrite_grid: (workgroups over the vectors of a row, workgroups over groups of four variants)"""
    gx = max(1, min((nvec + K["kRewriteVecs"] - 1) // K["kRewriteVecs"], K["kRewriteGroups"]))
    gy = max(1, min((m + WAVES - 1) // WAVES, max(1, K["kRewriteGroups"] // gx)))
    return gx, gy


def row_turns(nvec, gx, per_turn):
    """per turn of the `t` loop of a rewrite kernel, the list of (workgroup, lane, vectors taken) with at least one vector:
    t = 64 blockIdx.x + lane, t += per_turn 64 gx; a lane takes vector t and, where per_turn = 2, t + 64 gx if that is a
    vector of the row (`two`)"""
    step = gx * WAVE
    turns, t0 = [], 0
    while True:
        turn = []
        for b in range(gx):
            for lane in range(WAVE):
                t = t0 + b * WAVE + lane
                if t < nvec:
                    turn.append((b, lane, 1 + int(per_turn == 2 and t + step < nvec)))
        if not turn:
            return turns
        turns.append(turn)
        t0 += per_turn * step


def variant_turns(m, gy):
    """turns of the `j` loop of a rewrite kernel that the first wave takes, and the number of variants of the last group of four"""
    return -(-m // (gy * WAVES)), (m - 1) % WAVES + 1


def byte_chunks(n, m, K):
    """the (j0, cnt) launches of k_impute_bytes"""
    cols_per = min(max(1, min(K["kBytesMaxCols"], (K["kBytesChunkMiB"] << 20) // n)), m)
    return [(j0, min(cols_per, m - j0)) for j0 in range(0, m, cols_per)]


def byte_sample_turns(n, K):
    """turns of the sample loop of k_impute_bytes that thread 0 of workgroup 0 takes"""
    gx = max(1, min((n + BYTES_THREADS - 1) // BYTES_THREADS, K["kBytesGroups"]))
    return -(-n // (gx * BYTES_THREADS))


def shapes(K):
    """name -> (n, m): the smallest sample counts past each threshold (plus a few samples, so that n is no multiple of 4 or
    of 16 where that matters), and the variant counts past the two variant thresholds"""
    lane_turn = WAVE * VEC * 4                              # samples of one vector per lane of a wave: 4096
    gx1 = K["kRewriteVecs"] * VEC * 4                       # samples that one workgroup in x covers: 16384
    return {
        "exactly one vector per lane": (lane_turn, 7),
        "second vector on some lanes": (lane_turn + 1, 7),
        "second t turn": (PER_TURN * lane_turn + 8, 7),
        "two workgroups in x": (gx1 + 19, 7),
        "variant stride and second byte chunk": (3, max(K["kRewriteGroups"] * WAVES, K["kBytesMaxCols"]) + 4),
        "sample stride of the bytes": (K["kBytesGroups"] * BYTES_THREADS + 3, 3),
    }


SHAPE_NAMES = tuple(shapes(kernel_constants()))


def special_columns(n, m, K):
    """(all-missing variants, complete variants) that `shape_matrix` places.  m >= 5: the columns of `edge_matrix`; a wide
    matrix also gets one of each kind on both sides of the variant stride of the rewrite kernels and of the first byte
    chunk"""
    if m < 5:
        return [], []
    allna, complete = [2, m - 1], [1]
    for edge in (K["kRewriteGroups"] * WAVES, K["kBytesMaxCols"]):
        if m > edge + 2:
            allna += [edge - 1, edge + 1]
            complete += [edge - 2, edge + 2]
    assert len(set(allna) | set(complete) | {3, 4}) == len(allna) + len(complete) + 2
    return allna, complete


def shape_matrix(n, m, K):
    """(FBM bytes n x m, number of variants without a call): seeded random calls with a third missing, as `edge_matrix`;
    m >= 5 keeps its special columns and adds those of `special_columns`.  No other variant is left without a call (with
    3 samples one in 27 would be: such a variant gets one call back), so the count is what this builder intends."""
    rng = np.random.default_rng(1000 * n + m)
    g = rng.integers(0, 3, (n, m)).astype(np.uint8)
    g[rng.random((n, m)) < 0.33] = 3
    bare = np.flatnonzero((g == 3).all(0))
    g[rng.integers(0, n, bare.size), bare] = rng.integers(0, 3, bare.size)
    allna, complete = special_columns(n, m, K)
    if m >= 5:
        for j in complete + [3, 4]:
            g[:, j] = rng.integers(0, 3, n)
        g[0, 3] = 3
        g[n - 1, 4] = 3
        g[:, allna] = 3
    return np.asfortranarray(g), len(allna)


# ---- a dword whose sixteen fields are all missing -----------------------------------------------------------------------------

FULL_N, FULL_COLUMN, FULL_MISSING = 100, 1, (16, 48)


def full_dword_matrix():
    """100 x 3 calls without a missing value except variant 1, whose samples 16 .. 47 (its dwords 1 and 2) are missing"""
    rng = np.random.default_rng(16)
    g = rng.integers(0, 3, (FULL_N, 3)).astype(np.uint8)
    g[FULL_MISSING[0]:FULL_MISSING[1], FULL_COLUMN] = 3
    return np.asfortranarray(g)


def pack_dwords(col):
    """a variant's row of the 2-bit image as dwords: field e of dword d (bits 2 e, 2 e + 1) is the code of sample 16 d + e,
    0 / 1 / 2 = call, 3 = missing; pad fields are zero"""
    code = np.zeros(round_up(col.size, 16), dtype=np.uint64)
    code[:col.size] = col
    return (code.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(1).astype(np.uint32)


def missing_mask(x):
    """impute_step.hpp's missing_mask: bit 2 e set iff field e is missing"""
    x = np.asarray(x, dtype=np.uint32)
    return x & (x >> np.uint32(1)) & np.uint32(0x55555555)


# ---- a plain statement of the three deterministic rules ---------------------------------------------------------------------

def numpy_statement(g, method):
    """zero / mode / mean0 on FBM bytes: counts -> value -> np.where.  (bytes, number of variants without a call)"""
    g = np.asarray(g, dtype=np.uint8)
    c0, c1, c2 = ((g == k).sum(0).astype(np.int64) for k in range(3))
    c = c0 + c1 + c2
    if method == "zero":
        fill = np.full(g.shape[1], 3)
    elif method == "mode":
        v = np.where(c1 > c0, 1, 0)
        v = np.where((v == 0) & (c2 > c0), 2, v)
        v = np.where((v == 1) & (c2 > c1), 2, v)
        fill = 4 + v
    elif method == "mean0":
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (c1 + 2.0 * c2) / c
        fill = np.where(c > 0, 4 + np.rint(np.where(c > 0, mean, 0.0)).astype(np.int64), 3)
    else:
        raise ValueError(method)
    return np.where(g == 3, fill[None, :].astype(np.uint8), g), int((c == 0).sum())
