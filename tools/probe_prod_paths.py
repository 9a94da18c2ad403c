"""Which kernel every streaming product takes, and what it returns: a fixed, seeded list of products and solves that between
them take every launch path of matvec.hip that small images reach (bigsnpr_amd/csrc/prod_plan.hpp).  Per product one line: the
kernel of ScaledOp.last_kernel() and a SHA-256 of the product and of the crossproduct; per solve the kernels of
bsn_bed_streaming_kernels, the pass counts and a SHA-256 of d, u, v.  Two trees that print the same lines take the same paths
to the same bits.

    python tools/probe_prod_paths.py                   every switch setting, each in a child process of its own
    python tools/probe_prod_paths.py --one BSN_NO_SMAJ  one setting in this process (e.g. under rocprofv3 --kernel-trace)

It tests nothing by itself: compare its output between two builds."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = ["default", "BSN_NO_SMAJ", "BSN_NO_TILED", "BSN_NO_SPARSE_PROD", "BSN_NA_SKIP=0", "BSN_NA_SKIP=1", "BSN_FORCE_NA_PLANE"]
PANELS = [(8, 2), (16, 2), (11, 2), (16, 3), (5, 7)]   # vectors x digit slices


def digest(*parts):
    import numpy as np
    h = hashlib.sha256()
    for p in parts:
        a = np.ascontiguousarray(p)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:20]


def payload_of(G):
    """G [n x m] in {0, 1, 2, 3 = missing} -> the .bed payload (variant-major, four samples per byte)"""
    import numpy as np
    n, m = G.shape
    nb = (n + 3) // 4
    c = np.zeros((4 * nb, m), dtype=np.uint8)
    c[:n] = np.array([3, 2, 0, 1], dtype=np.uint8)[G]
    c = c.reshape(nb, 4, m)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).T.copy().ravel()


def one(setting):
    import numpy as np
    import bigsnpr_amd as ba
    from bigsnpr_amd import _lib
    if setting != "default":
        k, _, v = setting.partition("=")
        os.environ[k] = v or "1"
    lib = _lib.load()

    def line(name, text):
        print("%-18s %-44s %s" % (setting, name, text), flush=True)

    def guarded(name, fn):
        try:
            fn()
        except Exception as e:   # (a refusal is a result too: both builds must refuse alike; a device error ends the run)
            if "HIP error" in str(e):
                raise
            line(name, "ERROR %s" % str(e)[:140])

    def products(dname, image, n, m, seed):
        rng = np.random.default_rng(seed)
        scattered = np.sort(rng.permutation(m)[: max(70, m * 3 // 4)])
        subsets = [("cols 0..", None, None), ("cols 64..", np.arange(64, m), None), ("cols scattered", scattered, None),
                   ("row subset", None, np.sort(rng.choice(n, max(2, n * 2 // 3), replace=False)))]
        for cname, ic, ir in subsets:
            mm, nn = (m if ic is None else ic.size), (n if ir is None else ir.size)
            ce, sa = rng.uniform(0.1, 1.9, mm), rng.uniform(0.3, 1.0, mm)
            for nv, S in PANELS:
                X, Yr = rng.normal(size=(mm, nv)), rng.normal(size=(nn, nv))

                def run():
                    op = ba.ScaledOp(image, ir, ic, ce, sa, slices=S)
                    Y = op.prod(ba.DeviceArray.from_numpy(X))
                    op.sync()
                    kern = op.last_kernel()
                    Z = op.cprod(ba.DeviceArray.from_numpy(Yr))
                    op.sync()
                    line("%s %s %dx%d" % (dname, cname, nv, S), "prod=%s sha=%s cprod sha=%s" % (kern, digest(Y.to_numpy()), digest(Z.to_numpy())))
                    op.close()
                guarded("%s %s %dx%d" % (dname, cname, nv, S), run)

    def solve(dname, gb, **kw):
        def run():
            r = ba.bed_randomSVD(gb, **kw)
            buf = C.create_string_buffer(8192)
            _lib.check(lib.bsn_bed_streaming_kernels(gb.handle, buf, 8192))
            line("%s bed_randomSVD %s" % (dname, " ".join("%s=%s" % kv for kv in sorted(kw.items()))),
                 "nops=%d n_cprod=%d n_prod=%d wide=%d warm=%d na_skip=%d sha=%s %s"
                 % (r["nops"], r["n_cprod"], r["n_prod"], r["wide_steps"], r["warm_launches"], r["na_skip"], digest(r["d"], r["u"], r["v"]),
                    " ".join(buf.value.decode().split("\n"))))
        guarded("%s bed_randomSVD" % dname, run)

    rng = np.random.default_rng(77)
    # --- 2-bit images from a payload: 1 % missing, and the same complete
    n, m = 3001, 5003
    G = rng.integers(0, 3, (n, m)).astype(np.uint8)
    Gna = G.copy()
    Gna[rng.random((n, m)) < 0.01] = 3
    for dname, g in (("3001x5003 na", Gna), ("3001x5003 complete", G)):
        gb = ba.bed.from_payload(payload_of(g), n, m)
        gb.sample_major()
        products(dname, gb, n, m, seed=1)
        solve(dname, gb, k=5)
        solve(dname, gb, k=5, block=16)
        gb.close()
    # --- synthetic images (population structure, 1 % missing)
    for n, m, seed in ((1800, 3100, 5), (2500, 4096, 6), (640, 270000, 7)):
        gb = ba.bed.synthetic(n, m, seed=seed)
        gb.sample_major()
        if m == 3100:
            gb.tile()   # (the streaming-layout copy: the tiled instances of k_cprod / k_prod, unless BSN_NO_TILED)
        dname = "%dx%d" % (n, m)
        if m < 100000:
            products(dname, gb, n, m, seed=seed)
        else:   # (the wide image: whole-range products only, and the solve that has a warm start)
            for nv, S in PANELS:
                def run():
                    r2 = np.random.default_rng(nv * S)
                    op = ba.ScaledOp(gb, None, None, r2.uniform(0.1, 1.9, m), r2.uniform(0.3, 1.0, m), slices=S)
                    Y = op.prod(ba.DeviceArray.from_numpy(r2.normal(size=(m, nv))))
                    op.sync()
                    kern = op.last_kernel()
                    Z = op.cprod(ba.DeviceArray.from_numpy(r2.normal(size=(n, nv))))
                    op.sync()
                    line("%s cols 0.. %dx%d" % (dname, nv, S), "prod=%s sha=%s cprod sha=%s" % (kern, digest(Y.to_numpy()), digest(Z.to_numpy())))
                    op.close()
                guarded("%s cols 0.. %dx%d" % (dname, nv, S), run)
        solve(dname, gb, k=5, block=16)
        gb.close()
    # --- byte image (dosage grid), without and with missing values
    n, m = 300, 700
    dos = rng.integers(7, 208, size=(n, m)).astype(np.uint8)
    dos_na = dos.copy()
    dos_na[rng.random(dos.shape) < 0.03] = 3
    for dname, d in (("byte 300x700", dos), ("byte 300x700 na", dos_na)):
        Gf = ba.FBM_code256(d, ba.CODE_DOSAGE)
        products(dname, Gf._bed, n, m, seed=9)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        return one(sys.argv[2])
    names = {s.partition("=")[0] for s in SETTINGS}
    env = {k: v for k, v in os.environ.items() if k not in names}
    for s in SETTINGS:   # a fresh process per setting: no call under one setting precedes a call under another
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", s], env=env, cwd=ROOT, timeout=900)
        if r.returncode != 0:
            sys.exit("setting %s: exit status %d" % (s, r.returncode))   # (nothing more is started on the device)


if __name__ == "__main__":
    main()
