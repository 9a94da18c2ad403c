"""snp_ancestry_summary / bed_ancestry at the reference's shapes -> profiles/ancestry_c3.json.

What it records (device milliseconds are HIP events inside the library, bsn_ancestry_last_ms):

* snp_ancestry_summary at M = 5 000 000 variants, K = 21 groups, L = 16 loadings, one frequency vector: the call on host
  matrices (upload included), then the moment pass alone on resident matrices — repeated, with the spread — as bytes read
  once ((L + K + B) M doubles) over its time, beside the 6.3 TB/s a streaming read reaches on this device and the 8 TB/s
  of the data sheet; the same with the slab count forced (BSN_ANC_SLABS), alternating, equal results asserted within the
  reordering bound — an A/B for the record, no decision is taken from it; the CPU statement
  (tests/native/ancestry_ref.cpp, OpenMP) on the same tables.
* bed_ancestry at 50 000 samples x 200 000 variants of a synthetic image, K = 21, L = 16: device ms of the genotype pass
  (product against L + K + 2 columns and row norms), of the moment pass and of the program kernel; the same product pass
  through the existing bsn_bed_project_pca entry on the same columns as the comparison; the CPU statement on a subset of
  rows, its time SCALED to all rows (labelled as scaled).

No time here is a target.

    python tools/probe_ancestry.py [--M 5000000] [--n 50000] [--m 200000] [--cpu-rows 64] [--out profiles/ancestry_c3.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
import numpy as np  # noqa: E402

import bigsnpr_amd as ba  # noqa: E402
from bigsnpr_amd import _lib  # noqa: E402
from bigsnpr_amd._lib import check, f64p, ptr  # noqa: E402
from bigsnpr_amd.prs import project_last_ms  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.3e12, 8.0e12
K, L = 21, 16


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def timed(f):
    t0 = time.perf_counter()
    res = f()
    return res, time.perf_counter() - t0


def tables(M, seed):
    """reference frequencies with population structure, loadings of the size a PCA of M variants gives, a planted mixture"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.05, 0.95, size=M)
    X0 = np.asfortranarray(np.clip(base[:, None] + 0.08 * rng.standard_normal((M, K)), 0.0, 1.0))
    P = np.asfortranarray(rng.standard_normal((M, L)) / np.sqrt(M))
    w = np.zeros(K)
    w[[0, 7, 15]] = 0.6, 0.3, 0.1
    return X0, P, np.ones(L), w


def moments_resident(d_P, d_X0, d_F, M, B):
    out = dict(PtX0=np.zeros((L, K), order="F"), PtF=np.zeros((L, B), order="F"), G0=np.zeros((K, K), order="F"),
               X0tF=np.zeros((K, B), order="F"), csX0=np.zeros(K), csF=np.zeros(B), sqF=np.zeros(B))
    check(_lib.load().bsn_ancestry_moments(d_P.ptr, M, d_X0.ptr, M, d_F.ptr, M, M, L, K, B, 1,
                                           *[ptr(out[k], f64p) for k in ("PtX0", "PtF", "G0", "X0tF", "csX0", "csF", "sqF")]))
    return out, float(ba.ancestry_last_ms()[1])


def summary_part(a, rec):
    import ancestry_ref
    M = a.M
    X0, P, corr, w = tables(M, 1)
    F = X0 @ w
    ba.snp_ancestry_summary(F[:4096], X0[:4096], P[:4096], corr)            # first use of the library and of its buffers
    res, first = timed(lambda: ba.snp_ancestry_summary(F, X0, P, corr))
    res, call = timed(lambda: ba.snp_ancestry_summary(F, X0, P, corr))
    rec["summary"] = dict(M=M, K=K, L=L, B=1, first_call_s=first, call_s=call, call_note="host matrices in: the upload of "
                          "%.2f GB is part of the call; ms[1] adds the two moment passes of a call (tables alone, then with freq)"
                          % ((K + L + 1) * M * 8 / 1e9), device_ms=dict(zip(("genotype", "moments", "qp"), map(float, res.ms))),
                          steps=int(res.steps), cor_pred=float(res.cor_pred), max_err_vs_planted=float(np.abs(res.unrounded - w).max()))
    print("summary", json.dumps(rec["summary"]), flush=True)
    _write(a.out, rec)

    d_P, d_X0, d_F = (_lib.DeviceArray.from_numpy(x) for x in (P, X0, F))
    bytes_once = (L + K + 1) * M * 8.0
    sweep = {}
    base = None
    os.environ.pop("BSN_ANC_SLABS", None)
    moments_resident(d_P, d_X0, d_F, M, 1)
    for rnd in range(a.repeats):                                            # alternating: every variant in every round
        for s in [0] + list(a.slabs):
            if s:
                os.environ["BSN_ANC_SLABS"] = str(s)
            else:
                os.environ.pop("BSN_ANC_SLABS", None)
            out, ms = moments_resident(d_P, d_X0, d_F, M, 1)
            sweep.setdefault(s, []).append(ms)
            if base is None:
                base = out
            for k in base:
                assert np.allclose(out[k], base[k], rtol=1e-9, atol=0), (s, k)
    os.environ.pop("BSN_ANC_SLABS", None)
    for d in (d_P, d_X0, d_F):
        d.free()
    rec["moment_pass"] = dict(bytes_read_once=bytes_once, rule_slabs=int(-(-M // ancestry_ref.slab_rows())), runs=[
        dict(forced_slabs=s or None, ms=v, ms_median=float(np.median(v)), TBps=bytes_once / (np.median(v) * 1e-3) / 1e12,
             share_of_measured_streaming_read_6p3TBps=bytes_once / (np.median(v) * 1e-3) / HBM_MEASURED,
             share_of_spec_8TBps=bytes_once / (np.median(v) * 1e-3) / HBM_SPEC) for s, v in sweep.items()],
        note="A/B for the record: the rule (slabs of 4096 rows) stays; no decision was taken from these times")
    print("moment_pass", json.dumps(rec["moment_pass"]), flush=True)
    _write(a.out, rec)

    Dmat, _ = ba.nearPD((P.T @ X0).T @ (P.T @ X0))
    tw, cpu_s = timed(lambda: ancestry_ref.ancestry_summary(F, X0, P, corr, Dmat))
    rec["summary_cpu_twin"] = dict(threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None, seconds=cpu_s,
                                   max_abs_diff_w=float(np.abs(tw["w"][0] - res.unrounded).max()),
                                   ratio_to_device_ms=cpu_s / (sum(rec["summary"]["device_ms"].values()) * 1e-3))
    print("summary_cpu_twin", json.dumps(rec["summary_cpu_twin"]), flush=True)
    _write(a.out, rec)


def decode_rows(gb, rows):
    """allele counts (NaN = missing) of the first `rows` samples from the handle's .bed payload"""
    pay = gb.download()
    nb = (gb.nrow + 3) // 4
    by = np.asarray(pay, dtype=np.uint8).reshape(gb.ncol, nb)[:, : (rows + 3) // 4]
    codes = np.stack([(by >> s) & 3 for s in (0, 2, 4, 6)], axis=2).reshape(gb.ncol, -1)[:, :rows]
    return np.asfortranarray(np.array([2.0, np.nan, 1.0, 0.0])[codes].T)


def bed_part(a, rec):
    import ancestry_ref
    n, m = a.n, a.m
    gb = ba.bed.synthetic(n, m, seed=3)
    X0, P, corr, _ = tables(m, 2)
    ba.bed_ancestry(gb, X0, P, corr, ind_row=np.arange(1024), min_cor=-1)
    res, first = timed(lambda: ba.bed_ancestry(gb, X0, P, corr, min_cor=-1))
    res, call = timed(lambda: ba.bed_ancestry(gb, X0, P, corr, min_cor=-1))
    ms = dict(zip(("genotype", "moments", "qp"), map(float, res.ms)))
    nvec = L + K + 2
    rec["bed_ancestry"] = dict(n=n, m=m, K=K, L=L, first_call_s=first, call_s=call, device_ms=ms, product_columns=nvec,
                               image_GB=n * m / 4 / 1e9, steps_mean=float(res.steps.mean()), steps_max=int(res.steps.max()),
                               not_solved=int((res.steps == -2).sum()), cor_pred_median=float(np.nanmedian(res.cor_pred)))
    # the same product pass through the existing entry (bsn_bed_project_pca: product and row norms of the same columns)
    c = X0.mean(axis=1)
    V = np.asfortranarray(np.concatenate([P, X0, c[:, None], np.ones((m, 1))], axis=1))
    ba.project_pca(gb, None, None, 2.0 * c, np.full(m, 2.0), V, np.ones(nvec))
    ba.project_pca(gb, None, None, 2.0 * c, np.full(m, 2.0), V, np.ones(nvec))
    rec["bed_ancestry"]["existing_product_pass_ms_same_columns"] = float(project_last_ms()[0])
    print("bed_ancestry", json.dumps(rec["bed_ancestry"]), flush=True)
    _write(a.out, rec)

    if a.cpu_rows > 0:
        r = a.cpu_rows
        G = decode_rows(gb, r)
        Gf = np.where(np.isnan(G), 2.0 * c[None, :], G)
        Dmat, _ = ba.nearPD((P.T @ X0).T @ (P.T @ X0))
        tw, cpu_s = timed(lambda: ancestry_ref.ancestry_rows(Gf, X0, P, corr, Dmat))
        fo = lambda w: np.einsum("ik,kl,il->i", w, Dmat, w)   # noqa: E731  (the quadratic part: the weights may differ where D is flat)
        rec["bed_cpu_twin"] = dict(rows=r, threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None, seconds=cpu_s,
                                   max_abs_diff_cor_pred=float(np.abs(tw["cor_pred"] - res.cor_pred[:r]).max()),
                                   max_abs_diff_w=float(np.abs(tw["w"] - res.unrounded[:r]).max()),
                                   max_abs_diff_quadratic_form=float(np.abs(fo(tw["w"]) - fo(res.unrounded[:r])).max()),
                                   scaled_seconds_all_rows=cpu_s * n / r,
                                   scaled_note="SCALED by the number of rows from the run on %d; not run on all" % r,
                                   ratio_to_device_ms=cpu_s * n / r / (sum(ms.values()) * 1e-3))
        print("bed_cpu_twin", json.dumps(rec["bed_cpu_twin"]), flush=True)
        _write(a.out, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=5000000)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--m", type=int, default=200000)
    ap.add_argument("--cpu-rows", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slabs", type=int, nargs="+", default=[256, 512, 2048, 4096])
    ap.add_argument("--skip", choices=["summary", "bed"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ancestry_c3.json"))
    a = ap.parse_args()
    rec = dict(config="C3 ancestry", hbm_measured_streaming_read_Bps=HBM_MEASURED, hbm_spec_Bps=HBM_SPEC,
               note="nothing tuned: first shape of both kernels; device_ms are HIP events inside the library")
    if a.skip != "summary":
        summary_part(a, rec)
    if a.skip != "bed":
        bed_part(a, rec)


if __name__ == "__main__":
    main()
