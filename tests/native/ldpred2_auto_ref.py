"""The CPU statement of LDpred2-auto (ldpred2_auto_ref.cpp, over bigsnpr_amd/csrc/gibbs_auto.hpp) for the tests and
tools/probe_ldpred2_auto.py: built on first use with g++ -O2 -ffp-contract=off (OpenMP over chains when the compiler has
it), plus a short pure-Python restatement of the reference's loop that takes U, Z, the beta draws and the bootstrap
indices as arrays."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import ldpred2_ref as grid_ref
from ldpred2_ref import envelope, full_csc, full_from_upper, window_rows  # noqa: F401  (the same helpers)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "ldpred2_auto_ref.cpp")
HDRS = [os.path.join(ROOT, "bigsnpr_amd", "csrc", n) for n in ("gibbs_auto.hpp", "gibbs_step.hpp")]
SO = os.path.join(HERE, "libldpred2_auto_ref.so")
_lib = None

i64p, i32p, f64p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
MIN_H2 = 1e-3
SUM_THREADS = 256


def build():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        cxx = os.environ.get("CXX", "g++")
        base = [cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(HDRS[0]), SRC,
                "-o", SO + ".tmp"]
        try:
            subprocess.check_call(base[:1] + ["-fopenmp"] + base[1:])
        except subprocess.CalledProcessError:
            subprocess.check_call(base)
        os.replace(SO + ".tmp", SO)
    return SO


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(build())
        d, i, u64, u32, i64 = C.c_double, C.c_int, C.c_uint64, C.c_uint32, C.c_int64
        lib.lda_auto.restype = None
        lib.lda_auto.argtypes = [i64p, i32p, f64p, i64, f64p, f64p, f64p, i64, i64p, f64p, u64p, i64, d, i, i, i, i, d, i, d, d,
                                 d, d, d, u64, f64p, f64p, f64p, f64p, f64p, f64p, f64p, i32p, i64p, f64p, i]
        lib.lda_mle.restype = None
        lib.lda_mle.argtypes = [f64p, f64p, i64, d, d, f64p]
        lib.lda_sums.restype = None
        lib.lda_sums.argtypes = [f64p, f64p, i64, d, f64p]
        lib.lda_rbeta.restype = None
        lib.lda_rbeta.argtypes = [d, d, u64, u64, u32, i64, f64p]
        lib.lda_next_p.restype = d
        lib.lda_next_p.argtypes = [i64, i64, d, d, d, u64, u64, u32]
        lib.lda_boot_pick.restype = i64
        lib.lda_boot_pick.argtypes = [i64, d]
        lib.lda_boot.restype = None
        lib.lda_boot.argtypes = [i64, u64, u64, u32, i64p]
        lib.lda_tagged_sweep.restype = u32
        lib.lda_tagged_sweep.argtypes = [u32, u32]
        lib.lda_log.restype = d
        lib.lda_log.argtypes = [d]
        _lib = lib
    return _lib


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def auto(p, i, x, m2, beta_hat, n_vec, log_var, vec_p_init, h2_init, mean_ld, ind_sub=None, stream=None, burn_in=500,
         num_iter=200, report_step=None, no_jump_sign=False, shrink_corr=1.0, use_mle=True, p_bounds=(1e-5, 1.0),
         alpha_bounds=(-1.5, 0.5), seed=1, nthreads=0):
    """every chain of vec_p_init.  alpha_bounds are those of alpha (1 is added here, as R/LDpred2.R:254 does).  Returns a
    dict of arrays laid out as bsn_ldpred2_auto lays them out — beta_est, postp_est, corr_est [m x G] (beta_est NOT
    scaled back), sample_beta [m x n_report x G], path_p, path_h2, path_alpha [tot x G] — and path_nb [tot x G] (the
    size of the causal set after each sweep, -1 where the chain had stopped), moves [G], secs [G]"""
    L = load()
    p, i, x = np.ascontiguousarray(p, dtype=np.int64), np.ascontiguousarray(i, dtype=np.int32), _f64(x)
    bh, nv, lv, pi = _f64(beta_hat), _f64(n_vec), _f64(log_var), _f64(np.ravel(vec_p_init))
    sub = None if ind_sub is None else np.ascontiguousarray(ind_sub, dtype=np.int64)
    st = None if stream is None else np.ascontiguousarray(stream, dtype=np.uint64)
    m, G = bh.size, pi.size
    burn_in, num_iter = int(burn_in), int(num_iter)
    report_step = num_iter + 1 if report_step is None else min(int(report_step), num_iter + 1)
    tot, n_report = burn_in + num_iter, num_iter // report_step
    out = {k: np.empty((m, G), order="F") for k in ("beta_est", "postp_est", "corr_est")}
    out["sample_beta"] = np.empty((m, n_report, G), order="F")
    out.update({k: np.empty((tot, G), order="F") for k in ("path_p", "path_h2", "path_alpha")})
    out["path_nb"] = np.empty((tot, G), dtype=np.int32, order="F")
    out["moves"] = np.zeros(G, dtype=np.int64)
    out["secs"] = np.zeros(G)
    L.lda_auto(_ptr(p, i64p), _ptr(i, i32p), _ptr(x, f64p), int(m2), _ptr(bh, f64p), _ptr(nv, f64p), _ptr(lv, f64p), m,
               _ptr(sub, i64p), _ptr(pi, f64p), _ptr(st, u64p), G, float(h2_init), burn_in, num_iter, report_step,
               int(bool(no_jump_sign)), float(shrink_corr), int(bool(use_mle)), float(p_bounds[0]), float(p_bounds[1]),
               float(alpha_bounds[0]) + 1, float(alpha_bounds[1]) + 1, float(mean_ld), int(seed),
               _ptr(out["beta_est"], f64p), _ptr(out["postp_est"], f64p), _ptr(out["corr_est"], f64p),
               _ptr(out["sample_beta"], f64p), _ptr(out["path_p"], f64p), _ptr(out["path_h2"], f64p),
               _ptr(out["path_alpha"], f64p), _ptr(out["path_nb"], i32p), _ptr(out["moves"], i64p), _ptr(out["secs"], f64p),
               int(nthreads))
    return out


def mle(a, b, alpha1_bounds, par):
    """(alpha + 1, sigma2) minimising the objective over [alpha1_bounds] x [par[1] / 2, 2 par[1]]; len(a) == 0: par"""
    a, b = _f64(a), _f64(b)
    par = np.array(par, dtype=np.float64)
    load().lda_mle(_ptr(a, f64p), _ptr(b, f64p), a.size, float(alpha1_bounds[0]), float(alpha1_bounds[1]), _ptr(par, f64p))
    return par


def sums(a, b, alpha1):
    a, b = _f64(a), _f64(b)
    out = np.empty(3)
    load().lda_sums(_ptr(a, f64p), _ptr(b, f64p), a.size, float(alpha1), _ptr(out, f64p))
    return out


def rbeta(a, b, n, seed=1, stream=0, sweep0=0):
    out = np.empty(n)
    load().lda_rbeta(float(a), float(b), int(seed), int(stream), int(sweep0), n, _ptr(out, f64p))
    return out


def next_p(nb, m, mean_ld, p_bounds, seed, stream, sweep):
    return load().lda_next_p(int(nb), int(m), float(mean_ld), float(p_bounds[0]), float(p_bounds[1]), int(seed), int(stream),
                             int(sweep))


def boot_pick(nb, U):
    return load().lda_boot_pick(int(nb), float(U))


def boot(nb, seed, stream, sweep):
    out = np.empty(nb, dtype=np.int64)
    load().lda_boot(int(nb), int(seed), int(stream), int(sweep), _ptr(out, i64p))
    return out


def tagged_sweep(sweep, tag):
    return load().lda_tagged_sweep(int(sweep), int(tag))


def log_det(x):
    return load().lda_log(float(x))


# ---- pure Python ---------------------------------------------------------------------------------------------------------

def _exp(v):
    return float(grid_ref.exp_det([v])[0])


def py_sums(a, b, alpha1):
    """sum a, sum b exp(-alpha1 a), sum a b exp(-alpha1 a): 256 strided partial sums, then the pairwise tree"""
    part = [[0.0, 0.0, 0.0] for _ in range(SUM_THREADS)]
    for t in range(SUM_THREADS):
        for k in range(t, len(a), SUM_THREADS):
            ck = float(b[k]) * _exp(-alpha1 * float(a[k]))
            part[t][0] = part[t][0] + float(a[k])
            part[t][1] = part[t][1] + ck
            part[t][2] = part[t][2] + float(a[k]) * ck
    s = 1
    while s < SUM_THREADS:
        for t in range(0, SUM_THREADS, 2 * s):
            part[t] = [u + v for u, v in zip(part[t], part[t + s])]
        s *= 2
    return part[0]


def py_mle(a, b, alpha_lo, alpha_hi, par):
    """the minimiser of alpha1 sum_a + nb log(sigma2) + sum_k b_k exp(-alpha1 a_k) / sigma2 over the box, by bisection
    on the derivative of the profile in alpha1"""
    nb = len(a)
    if nb == 0:
        return list(par)
    lo, hi = par[1] / 2, par[1] * 2

    def at(al):
        sa, S, Sa = py_sums(a, b, al)
        sig = min(max(S / float(nb), lo), hi)
        return sa - Sa / sig, sig

    g, sig = at(alpha_lo)
    if not alpha_lo < alpha_hi or g >= 0:
        return [alpha_lo, sig]
    g, sig = at(alpha_hi)
    if g <= 0:
        return [alpha_hi, sig]
    x0, x1 = alpha_lo, alpha_hi
    for _ in range(64):
        mid = x0 + (x1 - x0) / 2
        if at(mid)[0] >= 0:
            x1 = mid
        else:
            x0 = mid
    al = x0 + (x1 - x0) / 2
    return [al, at(al)[1]]


def py_auto_one(p, i, x, m2, beta_hat, n_vec, log_var, ind_sub, p_init, h2_init, burn_in, num_iter, report_step,
                no_jump_sign, shrink_corr, use_mle, p_bounds, alpha1_bounds, U, Z, p_draws, boot_idx):
    """src/ldpred2-auto.cpp:57-202 in Python floats.  U, Z [(burn_in + num_iter) x m] stand for unif_rand() and norm_rand()
    of each (sweep, j); p_draws[k][nb] for Rf_rbeta after sweep k with nb causal variants (before the clamp is applied
    again, which changes nothing); boot_idx[k][nb] [nb] for the bootstrap's `nb * unif_rand()` of that sweep.  The MLE is
    py_mle.  Returns the reference's list (sample_beta dense)."""
    m = len(beta_hat)
    curr_beta, dotprods = [0.0] * m, [0.0] * m2
    avg_beta, avg_postp, avg_beta_hat = [0.0] * m, [0.0] * m, [0.0] * m
    tot = burn_in + num_iter
    sample_beta = np.zeros((m, num_iter // report_step))
    ind_report, next_k_reported = 0, burn_in + report_step - 1
    p_est, h2_est, alpha_est = (np.full(tot, np.nan) for _ in range(3))
    cur_h2_est = 0.0
    h2 = max(h2_init, MIN_H2)
    pp = min(max(p_bounds[0], p_init), p_bounds[1])
    par_mle = [0.0, h2 / (m * pp)]
    gap0 = 0.0
    for bj in beta_hat:
        gap0 = gap0 + float(bj) * float(bj)
    gap0 = 2 * gap0
    nan = np.full(m, np.nan)
    for k in range(tot):
        inv_odd_p = (1 - pp) / pp
        alpha_plus_one, sigma2 = par_mle
        gap = 0.0
        ind_causal = []
        for j in range(m):
            j2 = j if ind_sub is None else int(ind_sub[j])
            dotprod = dotprods[j2]
            n_j = float(n_vec[j])
            res_beta_hat_j = float(beta_hat[j]) - shrink_corr * (dotprod - curr_beta[j])
            scale_freq = _exp(alpha_plus_one * float(log_var[j])) if use_mle else 1
            C1 = scale_freq * sigma2 * n_j
            C2 = 1 / (1 + 1 / C1)
            C3 = C2 * res_beta_hat_j
            C4 = C2 / n_j
            postp = 1 / (1 + inv_odd_p * math.sqrt(1 + C1) * _exp(-C3 * C3 / C4 / 2))
            prev_beta = curr_beta[j]
            dotprod_shrunk = shrink_corr * dotprod + (1 - shrink_corr) * prev_beta
            if k >= burn_in:
                avg_postp[j] += postp
                avg_beta[j] += C3 * postp
                avg_beta_hat[j] += dotprod_shrunk
            diff = -prev_beta
            if postp > U[k][j]:
                samp_beta = C3 + math.sqrt(C4) * float(Z[k][j])
                if no_jump_sign and samp_beta * prev_beta < 0:
                    curr_beta[j] = 0.0
                else:
                    curr_beta[j] = samp_beta
                    diff += samp_beta
                    ind_causal.append(j)
                    gap += samp_beta * samp_beta
            else:
                curr_beta[j] = 0.0
            if diff != 0:
                cur_h2_est += diff * (2 * dotprod_shrunk + diff)
                for e in range(int(p[j2]), int(p[j2 + 1])):
                    r = int(i[e])
                    dotprods[r] = dotprods[r] + float(x[e]) * diff
        if gap > gap0:
            avg_beta, avg_postp, avg_beta_hat = nan, nan, nan
            break
        nb_causal = len(ind_causal)
        pp = min(max(p_bounds[0], float(p_draws[k][nb_causal])), p_bounds[1])
        h2 = max(cur_h2_est, MIN_H2)
        if use_mle:
            sel = [ind_causal[int(k2)] for k2 in boot_idx[k][nb_causal]]
            par_mle = py_mle([float(log_var[j]) for j in sel], [curr_beta[j] * curr_beta[j] for j in sel],
                             alpha1_bounds[0], alpha1_bounds[1], par_mle)
        else:
            par_mle = [par_mle[0], h2 / (m * pp)]
        p_est[k], h2_est[k] = pp, h2
        if use_mle:
            alpha_est[k] = par_mle[0] - 1
        if k == next_k_reported:
            for j in ind_causal:
                sample_beta[j, ind_report] = curr_beta[j]
            ind_report += 1
            next_k_reported += report_step
    return {"beta_est": np.asarray(avg_beta) / num_iter, "postp_est": np.asarray(avg_postp) / num_iter,
            "corr_est": np.asarray(avg_beta_hat) / num_iter, "sample_beta": sample_beta, "path_p_est": p_est,
            "path_h2_est": h2_est, "path_alpha_est": alpha_est}
