#!/usr/bin/env python3
"""knn_parallel / prob_dist / LOF at config C3's sample count -> profiles/knn_c3.json.

400 000 x 20 standard-normal scores scaled like the u of a partial SVD (unit columns).  Recorded:

* prob_dist (kNN = 5) and LOF (k = 30): the call on the host clock (upload of the scores and download of the result
  included) and the device times inside it (HIP events inside the library, bsn_knn_last_stats: packing pass, scan kernel,
  merge, the kernels after the table), with the slab count and the queries per workgroup the planner chose;
* the scan's 2 p n^2 fp64 vector operations (one subtraction and one fused multiply-add per coordinate and pair, the
  fused one counted once, as the vendor's peak counts an instruction per lane) over its time, beside the 78.6 TFLOP/s of
  the specification — that figure counts a fused multiply-add as two, so the share is also given with 3 p n^2;
* the CPU statement (tests/native/knn_ref.cpp, OpenMP) on a subset of the queries over all the data, compared bit for bit
  with the device's rows, and its time SCALED to all queries (labelled as scaled: the CPU did not run them all);
* knn_parallel with a small query set (1 000 queries over the 400 000 points, k = 30) with BSN_KNN_SLABS forced at a few
  values, so that the merge is timed — equal results asserted.

No time here is a target.

    python tools/probe_knn.py [--n 400000] [--p 20] [--cpu-queries 512] [--out profiles/knn_c3.json]
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

PEAK_F64_VECTOR = 78.6e12


def _write(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def timed(f):
    t0 = time.perf_counter()
    res = f()
    return res, time.perf_counter() - t0


def device_record(n, nq, p, call_s):
    st = ba.knn_last_stats()
    instr = 2.0 * p * n * nq
    scan_s = st["scan_ms"] * 1e-3
    return dict(call_s=call_s, device_ms=dict(pack=st["pack_ms"], scan=st["scan_ms"], merge=st["merge_ms"], rest=st["rest_ms"]),
                slabs=st["slabs"], query_block=st["query_block"], scan_vector_ops_2pn2=instr, scan_Tops=instr / scan_s / 1e12,
                share_of_f64_vector_peak_2pn2=instr / scan_s / PEAK_F64_VECTOR,
                share_of_f64_vector_peak_fma_as_two_3pn2=1.5 * instr / scan_s / PEAK_F64_VECTOR)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=400000)
    ap.add_argument("--p", type=int, default=20)
    ap.add_argument("--cpu-queries", type=int, default=512)
    ap.add_argument("--small-nq", type=int, default=1000)
    ap.add_argument("--slabs", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_c3.json"))
    a = ap.parse_args()
    os.environ.pop("BSN_KNN_SLABS", None)
    n, p = a.n, a.p
    U = np.random.default_rng(1).normal(size=(n, p)) / np.sqrt(n)
    rec = dict(config="C3 samples", n=n, p=p, peak_f64_vector_flops=PEAK_F64_VECTOR,
               note="nothing tuned: first shape of the kernel; call_s is the host clock of the second call (upload and download included)")

    ba.prob_dist(U[:4096], kNN=5)                      # first use of the library and of its buffers
    for name, f, k in (("prob_dist_kNN5", lambda: ba.prob_dist(U, kNN=5), 5), ("LOF_k30", lambda: ba.lof_matrix(U, (4, 10, 30)), 30)):
        _, first = timed(f)
        _, call = timed(f)
        rec[name] = dict(k=k, first_call_s=first, **device_record(n, n, p, call))
        print(name, json.dumps(rec[name]), flush=True)
        _write(a.out, rec)

    if a.cpu_queries > 0:
        import knn_ref
        rows = (n // 2, n // 2 + a.cpu_queries)
        want, cpu_s = timed(lambda: knn_ref.knn(U, None, 30, rows=rows))
        got = ba.knn_parallel(U, k=30)
        sl = slice(*rows)
        equal = np.array_equal(got["nn_idx"][sl], want["nn_idx"][sl]) and np.array_equal(got["nn_dists"][sl], want["nn_dists"][sl])
        rec["cpu_twin"] = dict(queries=a.cpu_queries, data_points=n, k=30, threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None,
                               seconds=cpu_s, rows_equal_to_device=bool(equal), scaled_seconds_all_queries=cpu_s * n / a.cpu_queries,
                               scaled_note="SCALED by the number of queries from the run on %d; not run on all" % a.cpu_queries,
                               ratio_to_device_scan=cpu_s * n / a.cpu_queries / (rec["LOF_k30"]["device_ms"]["scan"] * 1e-3))
        print("cpu_twin", json.dumps(rec["cpu_twin"]), flush=True)
        _write(a.out, rec)

    Q = U[: a.small_nq] * 1.0001
    rec["small_query_set"] = []
    base = None
    for s in [0] + list(a.slabs):
        os.environ["BSN_KNN_SLABS"] = str(s)
        ba.knn_parallel(U, Q, k=30)
        got, call = timed(lambda: ba.knn_parallel(U, Q, k=30))
        if base is None:
            base = got
        assert np.array_equal(got["nn_idx"], base["nn_idx"]) and np.array_equal(got["nn_dists"], base["nn_dists"])
        r = dict(nq=a.small_nq, k=30, forced_slabs=s if s > 0 else None, **device_record(n, a.small_nq, p, call))
        rec["small_query_set"].append(r)
        print("small", json.dumps(r), flush=True)
        _write(a.out, rec)
    os.environ.pop("BSN_KNN_SLABS", None)


if __name__ == "__main__":
    main()
