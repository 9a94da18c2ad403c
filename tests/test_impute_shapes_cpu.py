"""The inputs of tests/test_gpu_impute_shapes.py (tests/helpers/impute_inputs.py) without a GPU: each shape crosses the loop
of bigsnpr_amd/csrc/impute.hip it is named for — the thresholds are read from the source, the launch geometry is restated
in Python — and the CPU statement on it equals a plain numpy statement of zero / mode / mean0.  If a constant of the kernels
is retuned, the assertion that fails here names the shape that no longer covers its loop."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import impute_inputs as ii  # noqa: E402
import impute_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def K():
    k = ii.kernel_constants()
    assert set(k) == set(ii.CONSTANTS) and all(v > 0 for v in k.values())
    return k


@pytest.fixture(scope="module")
def S(K):
    return ii.shapes(K)


def _geometry(n, m, K):
    """both rewrite kernels and the byte kernel at n x m"""
    nvec2, nvec8 = ii.pitch2(n, K) // ii.VEC, ii.pitch8(n, K) // ii.VEC
    g2, g8 = ii.rewrite_grid(nvec2, m, K), ii.rewrite_grid(nvec8, m, K)
    return dict(nvec2=nvec2, nvec8=nvec8, g2=g2, g8=g8, t2=ii.row_turns(nvec2, g2[0], ii.PER_TURN), t8=ii.row_turns(nvec8, g8[0], 1),
                j2=ii.variant_turns(m, g2[1]), j8=ii.variant_turns(m, g8[1]), chunks=ii.byte_chunks(n, m, K),
                i_turns=ii.byte_sample_turns(n, K))


def test_the_image_never_hands_the_grid8_kernel_a_dword_past_the_source_row(K):
    """k_impute_grid8 reads dword t of the 2-bit row for every vector t of the int8 row"""
    for n in [1, 255, 256, 257, 1023, 1024, 1025] + [s[0] for s in ii.shapes(K).values()]:
        assert 4 * (ii.pitch8(n, K) // ii.VEC) <= ii.pitch2(n, K), n


def test_every_shape_crosses_the_loop_it_is_named_for(K, S):
    geo = {name: _geometry(n, m, K) for name, (n, m) in S.items()}
    for name, (n, m) in S.items():
        g = geo[name]
        print("%-40s %6d x %-6d 2-bit: %4d vectors, grid %s, %d t turns, %d j turns; int8: %5d vectors, grid %s, %d t turns; "
              "bytes: %d chunks, %d sample turns" % (name, n, m, g["nvec2"], g["g2"], len(g["t2"]), g["j2"][0], g["nvec8"],
                                                     g["g8"], len(g["t8"]), len(g["chunks"]), g["i_turns"]))

    def where(name, loop):
        return "%s (%d x %d) no longer covers: %s" % ((name,) + S[name] + (loop,))

    name = "exactly one vector per lane"
    g = geo[name]
    assert g["g2"][0] == 1 and len(g["t2"]) == 1 and len(g["t2"][0]) == ii.WAVE and all(k == 1 for _, _, k in g["t2"][0]), \
        where(name, "k_impute_2bit, every lane with one vector and `two` false on all of them")

    name = "second vector on some lanes"
    g = geo[name]
    took_two = [lane for _, lane, k in g["t2"][0] if k == 2]
    assert g["g2"][0] == 1 and len(g["t2"]) == 1 and 0 < len(took_two) < ii.WAVE and took_two == list(range(len(took_two))), \
        where(name, "k_impute_2bit, `two` true on the first lanes of a wave only")
    assert S[name][0] == S["exactly one vector per lane"][0] + 1, where(name, "the sample after the boundary")

    name = "second t turn"
    g = geo[name]
    assert g["g2"][0] == 1 and len(g["t2"]) >= 2 and len(g["t2"][0]) == ii.WAVE and all(k == 2 for _, _, k in g["t2"][0]), \
        where(name, "k_impute_2bit, a second turn of the t loop after a turn in which every lane took two vectors")

    name = "two workgroups in x"
    g = geo[name]
    n = S[name][0]
    assert g["g2"][0] == 2 and {b for b, _, _ in g["t2"][0]} == {0, 1}, where(name, "k_impute_2bit with gridDim.x = 2")
    assert g["g8"][0] > 2 and len(g["t8"]) >= 2, where(name, "k_impute_grid8 with gridDim.x > 1 and a second turn of its t loop")
    assert n % 4 != 0 and 0 < n % 16 < 4, where(name, "a last dword with fewer than four real samples; n no multiple of 4")
    assert ii.pitch8(n, K) - n > 0, where(name, "pad bytes behind the last sample of the int8 row")

    name = "variant stride and second byte chunk"
    g = geo[name]
    for kernel, grid, turns in (("k_impute_2bit", g["g2"], g["j2"]), ("k_impute_grid8", g["g8"], g["j8"])):
        assert grid[0] == 1 and grid[1] == K["kRewriteGroups"], where(name, kernel + " with gridDim.x = 1 and gridDim.y at its cap")
        assert turns[0] >= 2 and turns[1] < ii.WAVES, where(name, "the variant stride of %s, last group of four partial" % kernel)
    assert len(g["chunks"]) == 2 and g["chunks"][1][0] == K["kBytesMaxCols"] and 0 < g["chunks"][1][1] < K["kBytesMaxCols"], \
        where(name, "a second column chunk of the FBM bytes, cols_per at its cap")
    allna, complete = ii.special_columns(*S[name], K)
    for edge, what in ((g["g2"][1] * ii.WAVES, "the variant stride"), (g["chunks"][1][0], "the first byte chunk")):
        assert {edge - 1, edge + 1} <= set(allna) and {edge - 2, edge + 2} <= set(complete) and edge + 2 < S[name][1], \
            where(name, "all-missing and complete variants on both sides of %s" % what)

    name = "sample stride of the bytes"
    g = geo[name]
    assert g["i_turns"] >= 2 and len(g["chunks"]) == 1, where(name, "a second turn of the sample loop of k_impute_bytes")
    assert g["g2"][0] > 2 and g["g8"][0] > g["g2"][0], where(name, "many workgroups in x in both rewrite kernels")

    # below every threshold: what tests/test_gpu_impute.py reaches (n <= 3000, m <= 500)
    g = _geometry(3000, 500, K)
    assert len(g["t2"]) == 1 and all(k == 1 for _, _, k in g["t2"][0]) and g["j2"][0] == 1 and len(g["chunks"]) == 1 and g["i_turns"] == 1


@pytest.fixture(scope="module", params=ii.SHAPE_NAMES)
def built(request, K, S):
    n, m = S[request.param]
    g, n_all = ii.shape_matrix(n, m, K)
    return request.param, g, n_all


def test_the_builder_places_what_it_says(built, K):
    name, g, n_all = built
    n, m = g.shape
    assert g.flags.f_contiguous and g.dtype == np.uint8 and g.max() == 3
    assert 0.25 < (g == 3).mean() < 0.40, name                             # about a third missing
    allna, complete = ii.special_columns(n, m, K)
    assert sorted(np.flatnonzero((g == 3).all(0))) == sorted(allna) and n_all == len(allna), name
    assert not (g[:, complete] == 3).any(), name
    if m >= 5:
        assert list(np.flatnonzero(g[:, 3] == 3)) == [0] and list(np.flatnonzero(g[:, 4] == 3)) == [n - 1], name
        assert m - 1 in allna and 2 in allna and 1 in complete
    else:
        assert allna == [] and complete == []
    again, _ = ii.shape_matrix(n, m, K)
    assert np.array_equal(again, g)                                        # seeded


@pytest.mark.parametrize("method", ("zero", "mode", "mean0"))
def test_statement_equals_the_numpy_statement(built, method):
    name, g, n_all = built
    got, val, got_all = ref.impute(g, method, seed=ii.SEED, nthreads=4)
    want, want_all = ii.numpy_statement(g, method)
    assert np.array_equal(got, want), name
    assert got_all == want_all == n_all, name


@pytest.mark.parametrize("method", ("mean2", "random"))
def test_statement_leaves_calls_and_counts_the_rest(built, method):
    name, g, n_all = built
    got, val, got_all = ref.impute(g, method, seed=ii.SEED, nthreads=4)
    assert got_all == n_all and np.array_equal(got[g != 3], g[g != 3]), name
    allna = (g == 3).all(0)
    assert (got[:, allna] == 3).all() and (val[allna] == -1).all() and (val[~allna] >= 0).all(), name
    lo, hi = (7, 207) if method == "mean2" else (4, 6)
    filled = got[:, ~allna][g[:, ~allna] == 3]
    assert filled.min() >= lo and filled.max() <= hi, name


def test_full_dword_column():
    g = ii.full_dword_matrix()
    assert g.shape == (ii.FULL_N, 3)
    col = g[:, ii.FULL_COLUMN]
    lo, hi = ii.FULL_MISSING
    assert list(np.flatnonzero(col == 3)) == list(range(lo, hi)) and not (np.delete(g, ii.FULL_COLUMN, 1) == 3).any()
    masks = ii.missing_mask(ii.pack_dwords(col))
    assert list(masks) == [0, 0x55555555, 0x55555555, 0, 0, 0, 0]          # dwords 1 and 2: all sixteen fields, bit 30 included
    assert ii.pack_dwords(np.array([1, 2, 3, 0], dtype=np.uint8))[0] == 1 | (2 << 2) | (3 << 4)
    c1, c2, c = int((col == 1).sum()), int((col == 2).sum()), int((col < 3).sum())
    af = ref.rule_af(c1, c2, c)
    assert 0.2 < af < 0.8                                                   # the three calls all have a real chance
    out, val, n_all = ref.impute(g, "random", seed=ii.SEED)
    draws = np.array([ref.draw(ii.SEED, i, ii.FULL_COLUMN, af) for i in range(lo, hi)])
    assert n_all == 0 and np.array_equal(out[lo:hi, ii.FULL_COLUMN], 4 + draws) and np.unique(draws).size == 3
    assert draws[15] != draws[14] or draws[31] != draws[30] or draws[15] != draws[31]   # field 15 is not a copy of its neighbour
    out, val, _ = ref.impute(g, "mode", seed=ii.SEED)
    assert np.array_equal(out, ii.numpy_statement(g, "mode")[0]) and (out[lo:hi, ii.FULL_COLUMN] == 4 + val[ii.FULL_COLUMN]).all()


def test_the_draws_of_the_second_vector_tell_a_wrong_counter(K, S):
    """4097 x 7 has one sample in the second vector of a lane, sample 4096 (field 0 of lane 0's second vector).  A kernel
    that took the counter of that vector from the first (`tq = t`) would draw for sample 0 instead: with the seed of the
    tests the two draws differ on a variant where sample 4096 is missing, so `random` at this shape does not pass by luck."""
    name = "second vector on some lanes"
    n, m = S[name]
    g, _ = ii.shape_matrix(n, m, K)
    first = ii.WAVE * ii.VEC * 4
    assert n == first + 1
    told = []
    for j in np.flatnonzero(g[n - 1] == 3):
        c1, c2, c = int((g[:, j] == 1).sum()), int((g[:, j] == 2).sum()), int((g[:, j] < 3).sum())
        if c > 0 and ref.draw(ii.SEED, n - 1, j, ref.rule_af(c1, c2, c)) != ref.draw(ii.SEED, n - 1 - first, j, ref.rule_af(c1, c2, c)):
            told.append(int(j))
    print("variants whose draw at sample %d differs from the draw at sample 0: %s" % (n - 1, told))
    assert 4 in np.flatnonzero(g[n - 1] == 3) and told, "%s (%d x %d): no draw of the second vector differs from the first's" % (name, n, m)
