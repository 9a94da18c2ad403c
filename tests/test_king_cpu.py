"""bed_king without a device: the CPU statement (tests/native/king_ref.cpp over bigsnpr_amd/csrc/king_step.hpp — the header
the kernels use) against a NumPy restatement of the definition, the reference's expectations on the example data, and the
pruning rule king_norel."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import king_cases as kc  # noqa: E402
import king_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def example_table():
    return ref.table(kc.related_example())


@pytest.fixture(scope="module")
def missing_table():
    return ref.table(kc.read_golden("example-missing")[0])


def small_matrix():
    """37 x 301, 5 % missing, sample 5 without any heterozygous call, sample 11 entirely missing"""
    G = kc.random_codes(37, 301, 0.05, seed=20261019)
    G[5][G[5] == 1] = 2
    G[11] = 3
    return G


def test_twin_equals_numpy_example(example_table):
    kc.assert_same_table(example_table, kc.numpy_table(kc.related_example()))


def test_twin_equals_numpy_small():
    G = small_matrix()
    t = ref.table(G)
    kc.assert_same_table(t, kc.numpy_table(G))
    # ... and the plane identities against the counts taken by their definition
    np.testing.assert_array_equal(np.stack([t[c] for c in kc.COUNT_NAMES], axis=1), kc.direct_counts(G))
    kin = t["KINSHIP"]
    # the all-missing sample gives 0 / 0 with each of the 36 others; the sample without heterozygotes a zero denominator
    # under a positive numerator with each of the 35 others that have calls
    assert np.isnan(kin).sum() == 36
    assert np.isneginf(kin).sum() == 35
    assert np.isfinite(kin).sum() == 595
    assert not np.isposinf(kin).any()


def test_twin_equals_numpy_missing(missing_table):
    kc.assert_same_table(missing_table, kc.numpy_table(kc.read_golden("example-missing")[0]))


def test_reference_expectations(example_table):
    """tests/testthat/test-3-plink-QC.R:90-114 of the reference: one pair above 0.177, none above 0.3, IND2 removed"""
    from bigsnpr_amd.king import king_norel
    t = example_table
    order = np.argsort(-np.where(np.isfinite(t["KINSHIP"]), t["KINSHIP"], -np.inf), kind="stable")
    top = [(int(t["I1"][k]), int(t["I2"][k])) for k in order[:3]]
    assert top == [(0, 2), (0, 1), (168, 191)]
    k0, k1, k2 = order[:3]
    assert t["KINSHIP"][k0] == 0.18879387938793880 and t["HETHET"][k0] == 720 and t["IBS0"][k0] == 0
    assert t["KINSHIP"][k1] == 0.17349234923492352
    assert round(float(t["KINSHIP"][k2]), 4) == 0.1628
    assert (t["NSNP"] == 4542).all()
    one = ref.table(kc.related_example(), thr=0.177)
    assert one["KINSHIP"].size == 1 and one["KINSHIP"][0] > 0.177
    assert ref.table(kc.related_example(), thr=0.3)["KINSHIP"].size == 0
    keep, removed = king_norel(one, 517)
    assert removed.tolist() == [2] and keep.size == 516 and 2 not in keep
    fam = [line.split() for line in open(os.path.join(kc.GOLDEN, "example.fam"))]
    assert fam[2][:2] == ["POP1", "IND2"]


def test_example_missing_counts(missing_table):
    kin = missing_table["KINSHIP"]
    assert kin.size == 19900
    assert (~np.isfinite(kin)).sum() == 397
    assert ref.table(kc.read_golden("example-missing")[0], thr=2 ** -4.5)["KINSHIP"].size == 5689
    assert ref.table(kc.read_golden("example-missing")[0], thr=2 ** -3.5)["KINSHIP"].size == 4540


def test_payload_round_trip():
    G = kc.random_codes(13, 29, 0.1, seed=3)
    np.testing.assert_array_equal(kc.decode_payload(kc.encode_payload(G), 13, 29), G)


def test_norel_chain_tie_empty():
    from bigsnpr_amd.king import king_norel
    keep, removed = king_norel(dict(I1=[0, 1], I2=[1, 2]), 3)            # a - b - c: b goes
    assert removed.tolist() == [1] and keep.tolist() == [0, 2]
    keep, removed = king_norel(dict(I1=[3], I2=[5]), 7)                   # a tie: the larger index goes
    assert removed.tolist() == [5] and keep.tolist() == [0, 1, 2, 3, 4, 6]
    keep, removed = king_norel(dict(I1=np.zeros(0, dtype=np.int32), I2=np.zeros(0, dtype=np.int32)), 4)
    assert removed.size == 0 and keep.tolist() == [0, 1, 2, 3]
    # a triangle and a separate pair: every round takes the larger index among the most connected
    keep, removed = king_norel(dict(I1=[0, 0, 1, 4], I2=[1, 2, 2, 6]), 8)
    assert removed.tolist() == [2, 6, 1] and keep.tolist() == [0, 3, 4, 5, 7]
