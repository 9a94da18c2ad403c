"""Inputs of the big_spLinReg / big_spLogReg tests (tests/test_plr_cpu.py, tests/test_gpu_plr.py): the example data decoded on
the host, columns 0 .. 1499, four folds fixed by a seeded draw, and the phenotypes."""
import os

import numpy as np

N_COL = 1500
PATH = dict(nlambda=60, nlam_min=15, n_abort=5)


def y01_of(golden_dir):
    return np.array([int(line.split()[5]) for line in open(os.path.join(golden_dir, "example.fam"))]) - 1.0


def example_case(orc, golden_dir, example_bed):
    """X: 517 x 1500 doubles (the example data has no missing value); fold: ids 0 .. 3; ylin: every 400th column plus
    noise; y01: the .fam phenotype; ystrong / y01strong: phenotypes that a few columns explain almost entirely (for the
    optimality check, whose path must keep improving on the validation fold); read-only"""
    full = orc.read_bed(example_bed, na_val=3).astype(np.float64)
    assert full.shape == (517, 4542) and not (full == 3).any()
    X = np.asfortranarray(full[:, :N_COL])
    n = X.shape[0]
    rng = np.random.default_rng(2025)
    fold = rng.permutation(np.arange(n) % 4).astype(np.int32)
    causal = np.arange(0, N_COL, 400)
    eff = np.array([0.6, -0.5, 0.4, 0.5])
    ylin = X[:, causal] @ eff + rng.standard_normal(n)
    strong = np.array([10, 150, 300, 450, 590])
    lin = (X[:, strong] - X[:, strong].mean(axis=0)) @ np.array([1.0, -0.8, 0.9, 0.7, -1.1])
    ystrong = lin + 0.3 * rng.standard_normal(n)
    y01strong = (rng.random(n) < 1 / (1 + np.exp(-2.0 * lin))).astype(np.float64)
    out = dict(X=X, full=full, fold=fold, ylin=ylin, y01=y01_of(golden_dir), ystrong=ystrong, y01strong=y01strong)
    for v in out.values():
        v.setflags(write=False)
    return out
