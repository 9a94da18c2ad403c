"""The CPU statements of the BGEN path for the tests and tools/probe_bgen.py: inflate_ref.cpp (over
bigsnpr_amd/csrc/inflate_step.hpp) and bgen_ref.cpp (over bgen_step.hpp), built on first use with g++ -O2
-ffp-contract=off (OpenMP over streams when the compiler has it)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "bigsnpr_amd", "csrc")
HDRS = [os.path.join(CSRC, f) for f in ("inflate_step.hpp", "bgen_step.hpp", "gibbs_step.hpp")]
_libs = {}

u8p, i32p, i64p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


def build(name):
    src, so = os.path.join(HERE, name + ".cpp"), os.path.join(HERE, "lib%s.so" % name)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + HDRS):
        cxx = os.environ.get("CXX", "g++")
        base = [cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", CSRC, src, "-o", so + ".tmp"]
        try:
            subprocess.check_call(base[:1] + ["-fopenmp"] + base[1:])
        except subprocess.CalledProcessError:
            subprocess.check_call(base)
        os.replace(so + ".tmp", so)
    return so


def load(name):
    if name not in _libs:
        lib = C.CDLL(build(name))
        if name == "inflate_ref":
            lib.inflate_one_ref.restype = C.c_int
            lib.inflate_one_ref.argtypes = [u8p, C.c_int64, u8p, C.c_int64, C.c_int64]
            lib.inflate_ref.restype = None
            lib.inflate_ref.argtypes = [u8p, i64p, C.c_int64, u8p, i64p, i32p, C.c_int]
        else:
            lib.bgen_unit.restype = C.c_double
            lib.bgen_unit.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
            lib.bgen_random_call.argtypes = [C.c_double, C.c_int, C.c_int]
            lib.bgen_info_freq.restype = None
            lib.bgen_info_freq.argtypes = [C.c_int64, C.c_int64, C.c_int64, f64p]
            lib.bgen_variant_ref.restype = None
            lib.bgen_variant_ref.argtypes = [u8p, C.c_int64, i64p, C.c_int64, u8p, C.c_int, C.c_uint64, C.c_int64, u8p, i64p]
        _libs[name] = lib
    return _libs[name]


def inflate_one(stream, out_cap, expected_len):
    """(status, output bytes) of one stream through the statement"""
    a = np.frombuffer(bytes(stream) + b"\0", dtype=np.uint8).copy()
    out = np.zeros(max(int(out_cap), 1), dtype=np.uint8)
    st = load("inflate_ref").inflate_one_ref(a.ctypes.data_as(u8p), len(stream), out.ctypes.data_as(u8p), int(out_cap),
                                             int(expected_len))
    return int(st), out[:int(out_cap)].tobytes()


def inflate(inp, in_off, out_off, nthreads=1):
    """bsn_inflate's signature: (out, status)"""
    K = len(in_off) - 1
    out = np.zeros(max(int(out_off[-1]), 1), dtype=np.uint8)
    status = np.empty(K, dtype=np.int32)
    load("inflate_ref").inflate_ref(inp.ctypes.data_as(u8p), in_off.ctypes.data_as(i64p), K, out.ctypes.data_as(u8p),
                                    out_off.ctypes.data_as(i64p), status.ctypes.data_as(i32p), int(nthreads))
    return out[:int(out_off[-1])], status


def info_freq(nona, af, num):
    out = np.empty(2)
    load("bgen_ref").bgen_info_freq(int(nona), int(af), int(num), out.ctypes.data_as(f64p))
    return out[0], out[1]


def variant(block, N, ind_row, decode, dosage, seed, col):
    """(FBM bytes of the rows, (nona, af, num)) of one inflated block"""
    block = np.ascontiguousarray(block, dtype=np.uint8)
    ind_row = np.ascontiguousarray(ind_row, dtype=np.int64)
    decode = np.ascontiguousarray(decode, dtype=np.uint8)
    out, sums = np.empty(ind_row.size, dtype=np.uint8), np.empty(3, dtype=np.int64)
    load("bgen_ref").bgen_variant_ref(block.ctypes.data_as(u8p), int(N), ind_row.ctypes.data_as(i64p), ind_row.size,
                                      decode.ctypes.data_as(u8p), int(dosage), int(seed) & (2 ** 64 - 1), int(col),
                                      out.ctypes.data_as(u8p), sums.ctypes.data_as(i64p))
    return out, sums
