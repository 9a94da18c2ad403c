"""bed_ibd without a device: the CPU statement (tests/native/ibd_ref.cpp over bigsnpr_amd/csrc/ibd_step.hpp — the header the
kernels use) against a NumPy restatement of DESIGN.md 3.5p written here, the figures of the example data, the branches of
the estimate, and the pruning walk of indep_pairwise on hand-made pairs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ibd_cases as ic  # noqa: E402
import ibd_ref as ref  # noqa: E402
import king_cases as kc  # noqa: E402


@pytest.fixture(scope="module")
def example():
    G = kc.read_golden("example")[0]
    return G, ref.table(G)


@pytest.fixture(scope="module")
def missing():
    G = kc.read_golden("example-missing")[0]
    return G, ref.table(G)


def test_rows_of_the_moment_matrix_sum_to_one():
    """per variant a00 + a01 + a02 = 1 and a11 + a12 = 1: on both fixtures and on small counts, down to 2 called samples"""
    counts = [ic.variant_counts(kc.read_golden(name)[0]) for name in ("example", "example-missing")]
    small = np.array([(a, b, c) for a in range(6) for b in range(6) for c in range(6)])
    counts.append(small)
    n_used = 0
    for c in counts:
        a, used = ref.terms(c)
        np.testing.assert_array_equal(used, ic.numpy_terms(c)[1])
        assert (a[~used] == 0).all()
        assert np.abs(a[used, 0] + a[used, 1] + a[used, 2] - 1).max() <= 1e-12
        assert np.abs(a[used, 3] + a[used, 4] - 1).max() <= 1e-12
        n_used += int(used.sum())
    assert n_used > 4542 + 400
    # used iff more than 3 called alleles and both alleles seen
    _, used = ref.terms(np.array([[1, 0, 0], [1, 1, 0], [0, 2, 0], [2, 0, 0], [0, 0, 5], [0, 1, 1], [1, 0, 1]]))
    assert used.tolist() == [False, True, True, False, False, True, True]


@pytest.mark.parametrize("name", ["example", "example-missing", "small"])
def test_twin_equals_numpy(name, example, missing):
    if name == "small":
        G = ic.small_matrix()
        t = ref.table(G, freq=ic.small_freq())
        freq = ic.small_freq()
    else:
        G, t = example if name == "example" else missing
        freq = None
    want = ic.numpy_table(G, freq)
    for col in ("I1", "I2") + ref.IBS_NAMES:
        np.testing.assert_array_equal(t[col], want[col], err_msg=col)
    assert t["n_used"] == want["n_used"]
    np.testing.assert_allclose(t["E"], want["E"], rtol=1e-12, atol=0)
    # the estimate, bit for bit, when NumPy evaluates it from the twin's E in the stated order
    est = ic.numpy_estimate(np.stack([t[c] for c in ref.IBS_NAMES], axis=1), t["E"])
    for q, col in enumerate(ref.EST_NAMES):
        ic.assert_same_doubles(t[col], est[:, q], col)
    # ... and the twin's column entry gives what its table entry gives
    again = ref.estimate(np.stack([t[c] for c in ref.IBS_NAMES], axis=1), t["E"])
    for q, col in enumerate(ref.EST_NAMES):
        ic.assert_same_doubles(t[col], again[:, q], col)


def test_small_matrix_has_nan_rows_and_a_mask_that_bites():
    G, freq = ic.small_matrix(), ic.small_freq()
    t = ref.table(G, freq=freq)
    S = t["IBS0"] + t["IBS1"] + t["IBS2"]
    assert (S == 0).sum() == 36                      # the all-missing sample with each of the others
    for col in ref.EST_NAMES:
        np.testing.assert_array_equal(np.isnan(t[col]), S == 0)
    everyone = ref.table(G)
    assert 0 < t["n_used"] < everyone["n_used"] <= G.shape[1]
    assert (t["E"] != everyone["E"]).all()


def test_example_figures(example):
    G, t = example
    assert t["PI_HAT"].size == 133386 and t["n_used"] == 4542
    assert (t["IBS0"] + t["IBS1"] + t["IBS2"] == 4542).all()
    assert (t["PI_HAT"] >= 0.1).sum() == 426
    pi = np.sort(t["PI_HAT"])
    k = int(np.searchsorted(pi, 0.1))
    assert round(float(pi[k - 1]), 5) == 0.09990 and round(float(pi[k]), 5) == 0.10002
    assert abs(t["PI_HAT"].max() - 0.354032123650848) <= 1e-12
    np.testing.assert_allclose(t["E"], [0.08030495890854687, 0.454175795708235, 0.46551924538321815, 0.3876978156712112,
                                        0.6123021843287888], rtol=0, atol=1e-12)
    assert ref.table(G, min_pi_hat=0.1)["PI_HAT"].size == 426
    z = t["Z0"] + t["Z1"] + t["Z2"]
    assert np.abs(z - 1).max() < 1e-12 and (t["Z0"] >= 0).all() and (t["Z1"] >= 0).all() and (t["Z2"] >= 0).all()
    assert ((t["DST"] > 0) & (t["DST"] <= 1)).all()


def test_every_branch_fires_on_example_missing(missing):
    fired = missing[1]["fired"]
    for name in ("z0>1", "z1>1", "z2>1", "z1<0", "z2<0", "bounded"):
        assert fired[name] > 0, (name, fired)
    assert fired["z0<0"] == 0                          # ibs0 >= 0 and E00 > 0: z0 is never negative


def test_duplicate_sample_and_no_shared_call():
    G = kc.random_codes(12, 400, 0.0, seed=8)
    G[9] = G[4]
    assert 400 * (1.0 / 400) == 1.0                    # ibs2 * r is exactly 1 for this S (not for every S: DESIGN.md 3.5p)
    t = ref.table(G)
    k = int(np.flatnonzero((t["I1"] == 4) & (t["I2"] == 9))[0])
    assert (t["IBS0"][k], t["IBS1"][k], t["IBS2"][k]) == (0, 0, 400)
    assert (t["Z0"][k], t["Z1"][k], t["Z2"][k], t["PI_HAT"][k], t["DST"][k]) == (0.0, 0.0, 1.0, 1.0, 1.0)
    assert (np.delete(t["PI_HAT"], k) < 1).all()
    # S = 0: NaN in every double, by IEEE, and no filter passes it
    G[2, :200] = 3
    G[7, 200:] = 3
    t = ref.table(G)
    k = int(np.flatnonzero((t["I1"] == 2) & (t["I2"] == 7))[0])
    assert (t["IBS0"][k], t["IBS1"][k], t["IBS2"][k]) == (0, 0, 0)
    assert all(np.isnan(t[c][k]) for c in ref.EST_NAMES)
    assert sum(int(np.isnan(t[c]).sum()) for c in ref.EST_NAMES) == 5
    f = ref.table(G, min_pi_hat=0.0)
    assert f["PI_HAT"].size == t["PI_HAT"].size - 1 and not ((f["I1"] == 2) & (f["I2"] == 7)).any()


def test_moment_sum_order_is_leaf_then_top():
    """more than one leaf, the last one partial: the twin's E is the sum in the header's order, bit for bit"""
    G = kc.random_codes(40, 3 * ref.LEAF + 17, 0.05, seed=99)
    a, used = ref.terms(ic.variant_counts(G))
    top = np.zeros(5)
    for j0 in range(0, G.shape[1], ref.LEAF):
        leaf = np.zeros(5)
        for j in range(j0, min(j0 + ref.LEAF, G.shape[1])):
            leaf = leaf + a[j]
        top = top + leaf
    E, n_used = ref.moments(G)
    assert n_used == used.sum()
    ic.assert_same_doubles(E, top / float(n_used), "E")


def test_prune_walk_by_hand():
    from bigsnpr_amd.ibd import prune_walk
    # the smaller MAF goes
    assert prune_walk([0], [1], [0.1, 0.3]).tolist() == [False, True]
    assert prune_walk([0], [1], [0.3, 0.1]).tolist() == [True, False]
    # a tie: j goes
    assert prune_walk([0], [1], [0.2, 0.2]).tolist() == [True, False]
    # a removed i: (0, 1) removes 0, so (0, 2) is skipped although 2 has the smallest MAF of all; then (1, 2) removes 2
    assert prune_walk([0, 0], [1, 2], [0.1, 0.3, 0.05]).tolist() == [False, True, True]
    assert prune_walk([0, 0, 1], [1, 2, 2], [0.1, 0.3, 0.05]).tolist() == [False, True, False]
    # a removed j: (0, 2) removes 2, so (1, 2) is skipped and 1 stays although its MAF is smaller than 2's
    assert prune_walk([0, 1], [2, 2], [0.4, 0.01, 0.3]).tolist() == [True, True, False]
    # the order of the input does not matter: pairs are visited by (i, j)
    assert prune_walk([1, 0, 0], [2, 2, 1], [0.1, 0.3, 0.05]).tolist() == [False, True, False]
    # nothing in LD: everything stays
    assert prune_walk([], [], [0.1, 0.2, 0.3]).all()
    with pytest.raises(IndexError):
        prune_walk([1], [1], [0.1, 0.2])
    with pytest.raises(IndexError):
        prune_walk([0], [2], [0.1, 0.2])


def test_window_edge_and_two_chromosomes():
    """the pairs that reach the walk are those of the band j - i < window within a chromosome: ibd_cases.prune_rule builds
    them from a dense r^2 the way indep_pairwise builds them from bed_cor's entries, and walks them with prune_walk"""
    # five copies of one variant with falling MAF order 0 > 1 > 2 > 3 > 4 would all be in LD with each other
    r2 = np.ones((5, 5))
    maf = np.array([0.5, 0.4, 0.3, 0.2, 0.1])
    one = np.zeros(5, dtype=int)
    assert ic.prune_rule(r2, maf, one, window=5, thr_r2=0.2).tolist() == [True, False, False, False, False]
    # window 2: only neighbours; (0,1) removes 1, (2,3) removes 3, 4 has no partner left but (3,4) is skipped: 3 is gone
    assert ic.prune_rule(r2, maf, one, window=2, thr_r2=0.2).tolist() == [True, False, True, False, True]
    # window 3 reaches j - i = 2 and no further: with 0.1 r^2 between neighbours nothing but (i, i + 2) is in LD
    r2 = np.full((5, 5), 0.1)
    for i in range(3):
        r2[i, i + 2] = r2[i + 2, i] = 0.9
    assert ic.prune_rule(r2, maf, one, window=3, thr_r2=0.2).tolist() == [True, True, False, False, True]
    assert ic.prune_rule(r2, maf, one, window=2, thr_r2=0.2).all()
    # the threshold itself is not in LD (bed_cor keeps |r| > sqrt(thr_r2)), nor is NaN
    r2 = np.array([[1, 0.2, np.nan], [0.2, 1, np.nan], [np.nan, np.nan, 1]])
    assert ic.prune_rule(r2, np.array([0.3, 0.2, 0.1]), np.zeros(3, dtype=int), 3, 0.2).all()
    r2[0, 1] = r2[1, 0] = 0.21
    assert ic.prune_rule(r2, np.array([0.3, 0.2, 0.1]), np.zeros(3, dtype=int), 3, 0.2).tolist() == [True, False, True]
    # two chromosomes: no pair across the boundary, and positions count within the chromosome
    r2 = np.ones((6, 6))
    maf = np.array([0.1, 0.2, 0.3, 0.3, 0.2, 0.1])
    chrom = np.array([1, 1, 1, 2, 2, 2])
    assert ic.prune_rule(r2, maf, chrom, window=3, thr_r2=0.2).tolist() == [False, False, True, True, False, False]
    assert ic.prune_rule(r2, maf, np.ones(6, dtype=int), window=6, thr_r2=0.2).tolist() == [False, False, True, False, False, False]
