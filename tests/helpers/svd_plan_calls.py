"""The solve plan of bsn_bed_randomsvd (bigsnpr_amd/csrc/svd_plan.hpp) through tests/native: the layout of the fact and plan
vectors of nt_svd_plan / nt_svd_plan_resolve / nt_svd_needs_resolve / nt_svd_on_prodT and thin calls over them.  Used by
tests/test_svd_plan_cpu.py (the literal table) and tests/test_svd_driver_sweep_cpu.py (the automatic mode of the sweep)."""
import ctypes as C

import numpy as np

FACTS = ("k", "tol", "slices", "block", "vec_floor", "warm_start", "warm_denominator", "max_basis", "max_restarts", "seed", "verbose",
         "m", "m_total", "n", "cols_contig", "col0", "fused", "env_vec_floor_set", "env_vec_floor", "env_start_slices_set",
         "env_start_slices", "env_zq_split")
PLAN = ("k", "tol", "block", "slices_base", "slices_max", "vec_floor", "slices_start", "resid_floor", "noise_gain", "warm", "max_basis",
        "max_restarts", "seed", "verbose", "op_slices", "warm_on", "wants_smaj", "tile_ok")
# the default solve of a million variants over all ranks, 100 000 of them here in one 512-aligned range, 2 000 samples
BASE = dict(k=20, tol=1e-4, slices=0, block=0, vec_floor=0.0, warm_start=0, warm_denominator=0, max_basis=0, max_restarts=0, seed=0,
            verbose=0, m=100000, m_total=1000000, n=2000, cols_contig=1, col0=0, fused=0, env_vec_floor_set=0, env_vec_floor=0.0,
            env_start_slices_set=0, env_start_slices=0, env_zq_split=0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def facts(**kw):
    assert set(kw) <= set(FACTS)
    f = dict(BASE, **kw)
    return np.array([f[k] for k in FACTS], dtype=np.float64)


def plan_vec(p):
    return np.array([p[k] for k in PLAN], dtype=np.float64)


def plan(nt, **kw):
    out = np.zeros(len(PLAN))
    nt.nt_svd_plan(_p(facts(**kw)), _p(out))
    return dict(zip(PLAN, out.tolist()))


def resolve(nt, p):
    out = np.zeros(len(PLAN))
    nt.nt_svd_plan_resolve(_p(plan_vec(p)), _p(out))
    return dict(zip(PLAN, out.tolist()))


def on_prodT(nt, p, **kw):
    return nt.nt_svd_on_prodT(_p(facts(**kw)), _p(plan_vec(p)))


def needs_resolve(nt, exhausted, resid, below, p=None, **kw):
    p = p or plan(nt, **kw)
    return nt.nt_svd_needs_resolve(C.c_int(exhausted), C.c_double(resid), C.c_int(below), _p(facts(**kw)), _p(plan_vec(p)))
