"""The early Rayleigh-Ritz step of the SVD driver (svd_driver.hpp: early_grams / early_grams_wait / prefinalize) on the CPU:
tests/native/early_ritz_check.cpp drives block_lanczos_svd over a dense backend of its own, with the three hooks answering
and with them reporting "not supported", and compares d, u, v, niter and converged byte for byte — an ordinary solve, one
that restarts, a rank-deficient one (careful path) and one that converges at its first step — together with the order of
the hook calls and what becomes of every guess.  The program is built once plainly and once with
-fsanitize=address,undefined (runtimes linked statically: the program runs by itself whatever else the process environment preloads; nothing is
loaded into this interpreter)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "early_ritz_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                                                      "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_early_ritz_driver(tmp_path, flags):
    exe = str(tmp_path / "early_ritz_check")
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bigsnpr_amd", "csrc"),
                                             SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:]
    assert "all early Rayleigh-Ritz checks passed" in p.stdout, p.stdout[-4000:]
    assert "runtime error:" not in p.stdout and "AddressSanitizer" not in p.stdout, p.stdout[-4000:]
    for case in ("ordinary", "restart", "rank-deficient", "one-step"):
        assert case + ":" in p.stdout
