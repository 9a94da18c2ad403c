#!/usr/bin/env python3
"""snp_readBGEN / snp_prodBGEN at config C2 -> profiles/bgen_c2.json.

A written BGEN v1.2 file (layout 2, zlib level 6, 8 bits) with N = 50 000 samples, K = 4 096 variants and 90 % confident
calls: about 0.6 GB inflated.  Measured: the inflate kernel alone (HIP events inside the library, bsn_bgen_last_ms) as
output bytes over its time, the conversion to image rows, the product with 1 and with 16 columns, and each whole call (host
clock around the synchronous call, after a warm-up call, best and median of the repeats).  Yardsticks, reported and not
targets: zlib.decompress on one thread over the same streams in the same process, and the CPU twin
(tests/native/inflate_ref.cpp, the statement the kernel is compiled from) on 16 threads.  There is one window variant (the
LDS ring), so no A/B.  The device's bytes are compared with the decode through zlib on a subset of the variants.

    python tools/probe_bgen.py [--n 50000] [--k 4096] [--threads 16] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np  # noqa: E402

import bigsnpr_amd as ba  # noqa: E402
from bigsnpr_amd import _lib  # noqa: E402
import bgen_inputs as bi  # noqa: E402
import bgen_ref as ref  # noqa: E402


def last_ms():
    ms = (C.c_double * 3)()
    _lib.check(_lib.load().bsn_bgen_last_ms(ms))
    return list(ms)


def timed(f, repeats):
    f()
    t, ms = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
        ms.append(last_ms())
    best = int(np.argmin(t))
    return dict(call_s_best=t[best], call_s_median=float(np.median(t)), device_ms=ms[best])


def streams_of(path, offsets):
    raw = open(path, "rb").read()
    out = []
    for off in offsets:
        q = off
        for _ in range(3):
            q += 2 + struct.unpack_from("<H", raw, q)[0]
        q += 6
        for _ in range(2):
            q += 4 + struct.unpack_from("<I", raw, q)[0]
        c, = struct.unpack_from("<I", raw, q)
        out.append(raw[q + 8:q + 4 + c])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgen_c2.json"))
    a = ap.parse_args()
    N, K = a.n, a.k
    D = 10 + 3 * N
    with tempfile.TemporaryDirectory(prefix="probe_bgen_") as tmp:
        run(a, N, K, D, os.path.join(tmp, "c2.bgen"))


def run(a, N, K, D, path):
    t0 = time.perf_counter()
    parts = [bi.probabilities(N, min(256, K - j), seed=2 + j, missing=0.001, confident=0.9) for j in range(0, K, 256)]
    p0, p1, miss = (np.concatenate([p[k] for p in parts], axis=1) for k in range(3))
    del parts
    var = bi.write_bgen(path, p0, p1, miss)
    write_s = time.perf_counter() - t0
    ids = [[v["snp_id"] for v in var]]
    offs = [v["offset"] for v in var]
    z = streams_of(path, offs)
    rec = dict(config=dict(N=N, K=K, D=D, inflated_bytes=K * D, compressed_bytes=sum(len(s) for s in z), confident=0.9,
                           zlib_level=6, window="32-KiB ring in LDS, one wave per stream (the only variant built)"),
               write_file_s=write_s)

    t0 = time.perf_counter()
    for s in z:
        zlib.decompress(s)
    rec["zlib_1_thread"] = dict(s=time.perf_counter() - t0)
    rec["zlib_1_thread"]["GBps_out"] = K * D / rec["zlib_1_thread"]["s"] / 1e9
    inp, in_off, out_off = bi.pack(z, [D] * K)
    ref.inflate(inp, in_off[:9], out_off[:9], nthreads=a.threads)   # builds and loads the twin
    t0 = time.perf_counter()
    _, status = ref.inflate(inp, in_off, out_off, nthreads=a.threads)
    rec["twin_%d_threads" % a.threads] = dict(s=time.perf_counter() - t0, failed=int((status != 0).sum()))
    rec["twin_%d_threads" % a.threads]["GBps_out"] = K * D / rec["twin_%d_threads" % a.threads]["s"] / 1e9

    holder = {}

    def read():
        holder["res"] = None
        holder["res"] = ba.snp_readBGEN(path, ids)

    r = timed(read, a.repeats)
    r["inflate_GBps_out"] = K * D / (r["device_ms"][0] * 1e-3) / 1e9
    r["convert_GBps_in"] = K * D / (r["device_ms"][1] * 1e-3) / 1e9
    rec["snp_readBGEN"] = r
    sub = np.arange(0, K, max(1, K // 64))
    got = ba.snp_readBGEN(path, [[ids[0][j] for j in sub]], return_bytes=True)
    rec["bytes_equal_zlib_decode_on_subset"] = bool(np.array_equal(got.bytes, bi.decode_file(path, [offs[j] for j in sub])[0]))
    holder.clear()
    for ncol in (1, 16):
        beta = np.random.default_rng(ncol).standard_normal((K, ncol))
        rec["snp_prodBGEN_%d" % ncol] = timed(lambda: ba.snp_prodBGEN(path, beta, ids), a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
