"""The statement of one zlib stream (bigsnpr_amd/csrc/inflate_step.hpp, the header k_inflate is compiled from) without a
GPU: its CPU twin (tests/native/inflate_ref.cpp) against zlib.decompress, byte for byte, on streams of every block type
and at the limits of lengths and distances; the fixed list of malformed streams, each with its own status; and the same
header as a stand-alone program under -fsanitize=address,undefined over 2000 fixed-seed mutations — which has to pass
before any malformed stream is handed to the device (tests/test_gpu_bgen.py)."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "native"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import bgen_inputs as bi  # noqa: E402
import bgen_ref as ref  # noqa: E402


@pytest.mark.parametrize("case", bi.corpus(), ids=[c[0] for c in bi.corpus()])
def test_valid_streams_equal_zlib(case):
    name, stream, content = case
    assert zlib.decompress(stream) == content
    st, out = ref.inflate_one(stream, len(content), len(content))
    assert st == 0 and out == content
    # more room than needed changes nothing; the expected length is what is checked
    st, out = ref.inflate_one(stream, len(content) + 5, len(content))
    assert st == 0 and out[:len(content)] == content


def test_corpus_covers_what_it_claims():
    """the block types and limits the list is there for, read off the streams themselves"""
    by = {c[0]: c for c in bi.corpus()}
    assert (by["level0"][1][2] >> 1) & 3 == 0 and (by["fixed"][1][2] >> 1) & 3 == 1 and (by["level6"][1][2] >> 1) & 3 == 2
    assert len(by["two_stored_blocks"][2]) > 65535
    assert b"\x00\x00\xff\xff" in by["full_flush"][1]           # the empty stored block of Z_FULL_FLUSH
    assert [len(by["bytes%d" % n][2]) for n in (1, 13, 63, 64, 65)] == [1, 13, 63, 64, 65]
    assert len(by["dist32768"][2]) > 32768 + 258


def test_fixture_streams(tmp_path):
    """the reference's example file: 199 variants x 500 samples, every stream opens with a dynamic block, and the
    statement gives what zlib gives"""
    bgen = bi.example_files(tmp_path)
    raw = open(bgen, "rb").read()
    import sqlite3
    db = sqlite3.connect(bgen + ".bgi")
    offs = [r[0] for r in db.execute("SELECT file_start_position FROM Variant")]
    db.close()
    assert len(offs) == 199
    for off in offs:
        q = off
        for _ in range(3):
            q += 2 + struct.unpack_from("<H", raw, q)[0]
        q += 6
        for _ in range(2):
            q += 4 + struct.unpack_from("<I", raw, q)[0]
        C, D = struct.unpack_from("<II", raw, q)
        z = raw[q + 8:q + 4 + C]
        assert D == 10 + 3 * 500 and (z[2] >> 1) & 3 == 2
        st, out = ref.inflate_one(z, D, D)
        assert st == 0 and out == zlib.decompress(z)


@pytest.mark.parametrize("case", bi.malformed(), ids=[c[0] for c in bi.malformed()])
def test_malformed_streams_have_their_status(case):
    name, stream, cap, expected, status = case
    assert ref.inflate_one(stream, cap, expected)[0] == status


def test_many_streams_at_once():
    streams = [c[1] for c in bi.corpus()] + [m[1] for m in bi.malformed() if m[2] == m[3]]
    lens = [len(c[2]) for c in bi.corpus()] + [m[2] for m in bi.malformed() if m[2] == m[3]]
    want = [0] * len(bi.corpus()) + [m[4] for m in bi.malformed() if m[2] == m[3]]
    inp, in_off, out_off = bi.pack(streams, lens)
    out, status = ref.inflate(inp, in_off, out_off, nthreads=4)
    assert list(status) == want
    for k, c in enumerate(bi.corpus()):
        assert out[out_off[k]:out_off[k + 1]].tobytes() == c[2]


def test_header_under_a_sanitizer(tmp_path):
    """2000 fixed-seed mutations of valid streams plus the malformed list, every buffer allocated exactly, as a
    stand-alone program built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "inflate_fuzz")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "bigsnpr_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "inflate_fuzz.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the compiler cannot link the sanitizers: " + built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    items = [(c[1], len(c[2]), len(c[2]), 0) for c in bi.corpus() if len(c[2]) <= 6000]
    items += [(m[1], m[2], m[3], m[4]) for m in bi.malformed()]
    blob = struct.pack("<I", len(items))
    for s, cap, exp, status in items:
        blob += struct.pack("<IIIi", len(s), cap, exp, status) + s
    path = tmp_path / "streams.bin"
    path.write_bytes(blob)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "failures 0" in out.stdout
    hist = [int(x) for x in out.stdout.split("mutations by status:")[1].splitlines()[0].split()]
    assert sum(hist) == 2000 and sum(1 for h in hist if h) >= 4, hist   # the mutations reach several ways of failing
