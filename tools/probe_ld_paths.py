"""Which kernel every windowed-LD call takes, and what it returns: a fixed, seeded list of calls that between them
report every kernel id of bsn_ld_last_stats reachable without a 4-million-sample image (bigsnpr_amd/csrc/ld_plan.hpp,
DESIGN.md 3.6).  Per call one line: kernel, launches, tile_pairs, pairs of ld.last_stats() and a SHA-256 of every
returned array.  Two trees that print the same lines take the same paths to the same bits.

    python tools/probe_ld_paths.py                  every switch setting, each in a child process of its own
    python tools/probe_ld_paths.py --one BSN_LD_I8  one setting in this process (e.g. under rocprofv3 --kernel-trace)

It tests nothing by itself: compare its output between two builds."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = ["default", "BSN_LD_LUT", "BSN_LD_I8", "BSN_LD_NO_QUAD", "BSN_FORCE_NA_PLANE", "BSN_LD_BAND_BUDGET"]
BUDGET = "8000000"   # bytes: a band of 12 032 x 500 fp64 then goes in blocks of 1 920 columns


def digest(x):
    import numpy as np
    parts = x if isinstance(x, (tuple, list)) else (x,)
    h = hashlib.sha256()
    for p in parts:
        a = np.ascontiguousarray(p)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:24]


def one(setting):
    import numpy as np
    import bigsnpr_amd as ba
    from bigsnpr_amd import ld as ldm
    if setting != "default":
        os.environ[setting] = BUDGET if setting == "BSN_LD_BAND_BUDGET" else "1"
    rng = np.random.default_rng(2024)

    def csc(c):
        return (c.p, c.i, c.x)

    def report(name, fn):
        try:
            out = fn()
            st = ldm.last_stats()
            print("%-18s %-34s kernel=%-40.40s launches=%d tile_pairs=%d pairs=%d sha=%s"
                  % (setting, name, st["kernel"], st["launches"], st["tile_pairs"], st["pairs"], digest(out)), flush=True)
        except Exception as e:   # (a refusal is a result too: both builds must refuse alike; a device error ends the run)
            if "HIP error" in str(e):
                raise
            print("%-18s %-34s ERROR %s" % (setting, name, str(e)[:160]), flush=True)

    chunked = setting == "BSN_LD_BAND_BUDGET"   # (clumping holds its whole band: it refuses a budget it does not fit)
    # --- 2-bit image with missing values, few samples (no K split), many variants
    n, m = 500, 12032
    gb = ba.bed.synthetic(n, m, seed=7, na16=655)
    pos = np.arange(m, dtype=np.float64)
    chrom = np.repeat([1, 2], [7000, m - 7000])
    ir = np.sort(rng.choice(n, 400, replace=False))
    ic_small = np.arange(300, 1100)
    ic_scattered = rng.permutation(m)[:6000]
    report("na ld all-rows wide", lambda: ba.bed_ld_scores(gb, size=500, infos_pos=pos))
    report("na ld row-subset wide", lambda: ba.bed_ld_scores(gb, ind_row=ir, size=500, infos_pos=pos))
    report("na cor all-rows wide", lambda: csc(ba.bed_cor(gb, size=400, infos_pos=pos, alpha=0.5)))
    report("na cor narrow", lambda: csc(ba.bed_cor(gb, ind_col=ic_small, size=60, infos_pos=pos[ic_small], thr_r2=0.01)))
    report("na ld scattered columns", lambda: ba.bed_ld_scores(gb, ind_col=ic_scattered, size=300, infos_pos=np.arange(6000.0)))
    if not chunked:
        report("na bed_clumping wide", lambda: ba.bed_clumping(gb, thr_r2=0.02, size=400, infos_chr=chrom, infos_pos=pos * 1000))
        report("na bed_clumping row-subset", lambda: ba.bed_clumping(gb, ind_row=ir, thr_r2=0.1, size=400, infos_chr=chrom, infos_pos=pos * 1000))
        report("na bed_clumping narrow", lambda: ba.bed_clumping(gb, thr_r2=0.1, size=20, infos_chr=chrom, infos_pos=pos * 1000))
    # --- 2-bit image with missing values, enough samples for a K split, a narrow band
    n2, m2 = 2600, 900
    gk = ba.bed.synthetic(n2, m2, seed=8, na16=2000)
    pos2 = np.arange(m2, dtype=np.float64)
    report("na ld K-split", lambda: ba.bed_ld_scores(gk, size=50, infos_pos=pos2))
    report("na cor K-split scattered", lambda: csc(ba.bed_cor(gk, ind_col=rng.permutation(m2)[:500], size=40, infos_pos=np.arange(500.0))))
    # --- 2-bit image without missing values: the cross product alone
    n3, m3 = 1300, 2250
    gc = ba.bed.synthetic(n3, m3, seed=33, na16=0)
    pos3 = np.cumsum(rng.uniform(0.5, 1.5, m3))
    ir3 = np.sort(rng.choice(n3, 900, replace=False))
    report("complete ld all-rows", lambda: ba.bed_ld_scores(gc, size=0.3, infos_pos=pos3))
    report("complete ld row-subset", lambda: ba.bed_ld_scores(gc, ind_row=ir3, size=0.07, infos_pos=pos3))
    report("complete cor few pairs", lambda: csc(ba.bed_cor(gc, ind_col=np.arange(400), size=0.03, infos_pos=pos3[:400], thr_r2=0.001)))
    report("complete cor scattered", lambda: csc(ba.bed_cor(gc, ind_row=ir3, ind_col=rng.permutation(m3)[:1500], size=0.2, infos_pos=pos3[:1500])))
    codes = rng.integers(0, 3, size=(700, 1500)).astype(np.uint8)
    chr3 = np.repeat([1, 2, 3], 500)
    if not chunked:
        report("complete bed_clumping", lambda: ba.bed_clumping(gc, thr_r2=0.05, size=200, infos_chr=np.repeat([1, 2, 3], 750), infos_pos=1000.0 * np.arange(m3)))
        report("fbm snp_clumping complete", lambda: ba.snp_clumping(ba.FBM_code256(codes), chr3, thr_r2=0.05, size=200))
        holes = codes.copy()
        holes[rng.random(holes.shape) < 0.01] = 3
        report("fbm snp_clumping missing", lambda: ba.snp_clumping(ba.FBM_code256(holes), chr3, thr_r2=0.05, size=200))
    # --- dosage FBM (byte image), without and with missing values
    dos = rng.integers(7, 208, size=(900, 700)).astype(np.uint8)
    posd = np.cumsum(rng.integers(1, 3000, size=700)).astype(np.float64)
    G = ba.FBM_code256(dos, ba.CODE_DOSAGE)
    report("dosage cor", lambda: csc(ba.snp_cor(G, size=40, infos_pos=posd)))
    report("dosage ld row-subset", lambda: ba.snp_ld_scores(G, ind_row=np.arange(0, 900, 2), size=40, infos_pos=posd))
    dos_na = dos.copy()
    dos_na[rng.random(dos.shape) < 0.03] = 3
    Gn = ba.FBM_code256(dos_na, ba.CODE_DOSAGE)
    report("dosage-na cor", lambda: csc(ba.snp_cor(Gn, size=40, infos_pos=posd)))
    report("dosage-na ld", lambda: ba.snp_ld_scores(Gn, size=40, infos_pos=posd))
    if not chunked:
        report("dosage snp_clumping", lambda: ba.snp_clumping(G, np.repeat([1, 2], 350), thr_r2=0.2, infos_pos=posd))
        report("dosage-na snp_clumping", lambda: ba.snp_clumping(Gn, np.repeat([1, 2], 350), thr_r2=0.2, infos_pos=posd))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        return one(sys.argv[2])
    env = {k: v for k, v in os.environ.items() if k not in SETTINGS}
    for s in SETTINGS:   # a fresh process per setting: no call under one setting precedes a call under another
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", s], env=env, cwd=ROOT, timeout=900)
        if r.returncode != 0:
            sys.exit("setting %s: exit status %d" % (s, r.returncode))   # (nothing more is started on the device)


if __name__ == "__main__":
    main()
