"""snp_match and same_ref (bigsnpr_amd/match.py) on the small tables of the reference's match test
(tests/testthat/test-5-match.R:9-75; tables and expected results in tests/golden/snp_match_cases.json): matched counts,
the signs of beta, _FLIP_ and _REV_, the join by rsid, the duplicates case, the errors, the same_ref vector.  Row
numbers are 0-based here.  Pure host logic.

The fixture holds data only: the three tables of that test and what it expects of them (dimensions, signs of beta,
_FLIP_ / _REV_, messages, errors, the same_ref vector).  Its `same_ref_example` block is the input of the same_ref()
documentation example (R/match-alleles.R:152-155) with the values that the function's decision rules give — worked out
from the rules, not recorded from a run of the reference."""
import json
import os

import numpy as np
import pytest

from bigsnpr_amd.match import flip_strand, same_ref, snp_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "snp_match_cases.json")) as _f:
    CASES = json.load(_f)


def _dim(t):
    return [len(next(iter(t.values()))), len(t)]


def _rows(table, rows):
    n = max(len(v) for v in table.values() if isinstance(v, list))
    return {k: [v[i] for i in rows] if isinstance(v, list) else v for k, v in table.items()} if rows is not None else table, n


def test_strand_flip_and_reverse(capsys):
    want = CASES["strand_flip"]
    m = snp_match(CASES["sumstats"], CASES["info_snp"])
    assert want["message"] in capsys.readouterr().out
    assert _dim(m) == want["dim"]
    beta = np.array(CASES["sumstats"]["beta"])
    assert np.array_equal(m["_NUM_ID_.ss"], want["sumstats_rows"])
    assert np.array_equal(m["beta"], beta[want["sumstats_rows"]] * want["beta_sign"])
    assert "_FLIP_" not in m and "_REV_" not in m
    # rows are ordered by (chr, pos); the alleles are info_snp's
    assert np.all(np.diff(m["pos"]) > 0)
    assert np.array_equal(m["a0"], np.array(CASES["info_snp"]["a0"])[m["_NUM_ID_"]])

    m3 = snp_match(CASES["sumstats"], CASES["info_snp"], return_flip_and_rev=True)
    assert want["message"] in capsys.readouterr().out
    assert _dim(m3) == want["dim_with_flip_and_rev"]
    assert m3["_FLIP_"].tolist() == want["_FLIP_"] and m3["_REV_"].tolist() == want["_REV_"]


def test_without_strand_flip(capsys):
    want = CASES["no_strand_flip"]
    m = snp_match(CASES["sumstats"], CASES["info_snp"], strand_flip=False)
    out = capsys.readouterr().out
    assert want["message"] in out and "ambiguous" not in out
    assert _dim(m) == want["dim"]
    beta = np.array(CASES["sumstats"]["beta"])
    assert np.array_equal(m["_NUM_ID_.ss"], want["sumstats_rows"])
    assert np.array_equal(m["beta"], beta[want["sumstats_rows"]] * want["beta_sign"])


def test_verbose_prints_the_three_counts_and_can_be_silenced(capsys):
    snp_match(CASES["sumstats"], CASES["info_snp"])
    out = capsys.readouterr().out
    assert "6 variants to be matched." in out
    assert "1 ambiguous SNPs have been removed." in out      # T/A at 755890
    assert "4 variants have been matched; 1 were flipped and 1 were reversed." in out
    snp_match(CASES["sumstats"], CASES["info_snp"], verbose=False)
    assert capsys.readouterr().out == ""


def test_join_by_rsid():
    want = CASES["by_rsid"]
    ss2, info = CASES["sumstats2"], CASES["info_snp"]
    m = snp_match(ss2, info, join_by_pos=False, verbose=False)
    assert _dim(m) == want["dim"]
    assert m["beta"].tolist() == want["beta"]
    assert np.array_equal(m["pos.ss"], m["pos"] + want["pos_shift"])
    for c in want["info_columns"]:
        col = np.broadcast_to(np.asarray(info[c]), (5,))
        assert np.array_equal(m[c], col[m["_NUM_ID_"]]), c
    assert want["sumstats_columns"] == ["chr", "rsid", "beta"]
    assert np.array_equal(m["rsid"], np.array(ss2["rsid"], dtype=object)[m["_NUM_ID_.ss"]])
    assert np.all(m["chr"] == ss2["chr"]) and np.all(np.abs(m["beta"]) == ss2["beta"])


def test_every_row_of_a_duplicated_position_is_dropped(capsys):
    want = CASES["duplicates"]
    ss2, _ = _rows(CASES["sumstats2"], want["sumstats2_rows"])
    m = snp_match(ss2, CASES["info_snp"], join_by_pos=False)
    assert want["message"] in capsys.readouterr().out
    assert _dim(m) == want["dim"]
    assert 0 not in m["_NUM_ID_"]                   # not only the later of the two rows is gone
    kept = snp_match(ss2, CASES["info_snp"], join_by_pos=False, remove_dups=False, verbose=False)
    assert _dim(kept) == [5, 9] and (kept["_NUM_ID_"] == 0).sum() == 2


def test_errors_are_the_references():
    want = CASES["errors"]
    ss2, info = CASES["sumstats2"], CASES["info_snp"]
    no_beta = {k: v for k, v in ss2.items() if k != "beta"}
    with pytest.raises(ValueError, match=want["sumstats_names"]):
        snp_match(no_beta, info, verbose=False)
    no_pos = {k: v for k, v in info.items() if k != "pos"}
    with pytest.raises(ValueError, match=want["info_snp_names"]):
        snp_match(ss2, no_pos, verbose=False)
    with pytest.raises(ValueError, match=want["none_matched"]):
        snp_match(ss2, info, verbose=False)            # positions shifted by 10: nothing in common
    with pytest.raises(ValueError, match=want["not_enough"]):
        snp_match(CASES["sumstats"], info, match_min_prop=0.9, verbose=False)   # 4 matched < 0.9 * 5


def test_a_non_acgt_allele_has_no_flipped_twin():
    assert flip_strand(["A", "C", "G", "T", "AT", "N", None]) == ["T", "G", "C", "A", None, None, None]
    ss = dict(chr=[1, 1], pos=[10, 20], a0=["AT", "A"], a1=["A", "C"], beta=[1.0, 1.0])
    info = dict(chr=[1, 1], pos=[10, 20], a0=["A", "G"], a1=["AT", "T"])
    m = snp_match(ss, info, return_flip_and_rev=True, verbose=False)
    # the indel is matched reversed as it stands, A/C is matched reversed on the other strand
    assert m["_NUM_ID_"].tolist() == [0, 1]
    assert m["_REV_"].tolist() == [True, True] and m["_FLIP_"].tolist() == [False, True]
    assert m["beta"].tolist() == [-1.0, -1.0]


def test_same_ref():
    want = CASES["same_ref"]
    info, ss = CASES["info_snp"], CASES["sumstats"]
    r = want["rows"]
    got = same_ref([info["a1"][i] for i in r], [info["a0"][i] for i in r], [ss["a1"][i] for i in r], [ss["a0"][i] for i in r])
    assert got.tolist() == want["expected"]
    ex = CASES["same_ref_example"]
    assert same_ref(ex["ref1"], ex["alt1"], ex["ref2"], ex["alt2"]).tolist() == ex["expected"]
