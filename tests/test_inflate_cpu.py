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
    # the dynamic blocks that zlib's compressor does not make, read off the code lengths they were emitted from
    W, F, sp = 32768, 2048, bi.SPECS   # the ring of k_inflate and its kFlushBytes
    for name in ("dyn_lit15", "dyn_one_dist", "dyn_one_dist_29", "dyn_run_crosses", "dyn_two_tables"):
        assert (by[name][1][2] >> 1) & 3 == 2, name
        assert len(by[name][2]) == len(bi.apply_tokens(sp[name]["tokens"])), name
    s = sp["dyn_lit15"]
    assert max(s["lit_lens"]) == 15 and sorted(n for n in s["lit_lens"] if n) == list(range(1, 15)) + [15, 15]
    assert s["lit_lens"][256] == 15 and s["dist_lens"] == [0] and not bi.token_spans(s["tokens"])
    assert 77 in s["tokens"] and s["lit_lens"][77] == 15                # a literal of 15 bits is decoded, not only declared
    assert sp["dyn_one_dist"]["dist_lens"] == [1] and set(bi.token_spans(sp["dyn_one_dist"]["tokens"])) >= {(1, 3, 1)}
    assert {(n, d) for _, n, d in bi.token_spans(sp["dyn_one_dist"]["tokens"])} == {(3, 1)}
    s = sp["dyn_one_dist_29"]
    assert len(s["lit_lens"]) == 286 and len(s["dist_lens"]) == 30 and s["dist_lens"] == [0] * 29 + [1]
    assert bi.token_spans(s["tokens"]) == [(W, 258, 32768), (W + 258, 258, 24577)]
    s = sp["dyn_run_crosses"]
    assert s["cl_syms"] == [(1, 1), (18, 138), (18, 117), (2, 1), (16, 5)]
    run_from = 1 + 138 + 117 + 1          # the lengths written before the run of symbol 16: it fills [257, 262)
    assert run_from == 257 < len(s["lit_lens"]) == 258 < run_from + 5 == len(s["lit_lens"]) + len(s["dist_lens"])
    assert [(n, d) for _, n, d in bi.token_spans(s["tokens"])] == [(3, 1), (3, 2), (3, 3), (3, 4)]
    s = sp["dyn_two_tables"]
    assert s["lit_lens"] != s["lit_lens2"][:len(s["lit_lens"])]
    assert any(p >= s["first_block_bytes"] > p - d for p, n, d in bi.token_spans(s["tokens"]))
    # matches at the end of the ring: destination across 32 768; source across 32 768 with the destination across 65 536
    assert (by["ring_end_dest"][1][2] >> 1) & 3 == 1 and (by["ring_end_both"][1][2] >> 1) & 3 == 1
    assert any(p < W < p + n for p, n, d in bi.token_spans(sp["ring_end_dest"]["tokens"]))
    assert (32700, 258, 50) in bi.token_spans(sp["ring_end_dest"]["tokens"])
    assert any(p - d < W < p - d + n and p < 2 * W < p + n for p, n, d in bi.token_spans(sp["ring_end_both"]["tokens"]))
    assert bi.token_spans(sp["ring_end_both"]["tokens"])[-1] == (65406, 258, 32768)
    # flushes: a sink that flushes after a token once kFlushBytes wait.  The largest flush is 2 047 + 258 bytes: a match of
    # 258 that starts at pos % 2048 == 2047 with nothing flushed since pos - 2047; and a match that completes exactly 2 048
    toks = sp["flush_2305"]["tokens"]
    flushes = bi.flush_spans(toks, F)
    spans = bi.token_spans(toks)
    assert any(p % F == F - 1 and n == 258 and (p - (F - 1), p + n) in flushes for p, n, d in spans)
    assert max(b - a for a, b in flushes) == F - 1 + 258 == 2305
    assert any((p + n - F, p + n) in flushes and p > p + n - F for p, n, d in spans)
    assert all(b - a <= F - 1 + 258 for name in sp for a, b in bi.flush_spans(sp[name]["tokens"], F))
    # len = 258 at distances one below and one above a wave, and one above two and four waves
    assert {d for p, n, d in bi.token_spans(sp["periodic_258"]["tokens"]) if n == 258} == {63, 65, 129, 257}
    assert all(d <= p for name in sp for p, n, d in bi.token_spans(sp[name]["tokens"]))
    assert set(by["adler_ff"][2]) == {255} and 69000 < len(by["adler_ff"][2]) < 70000
    assert max(len(c[2]) for c in bi.corpus()) <= 70000


def test_deviations_zlib_accepts_and_the_statement_refuses():
    """the documented deviation (inflate_step.hpp): a literal/length set that holds only the end-of-block code"""
    assert [d[0] for d in bi.deviations()] == ["dyn_only_end_of_block"]
    for name, stream, cap, expected, status in bi.deviations():
        assert (stream[2] >> 1) & 3 == 2
        assert zlib.decompress(stream) == b"" and cap == expected == 0
        assert status == 4 and ref.inflate_one(stream, cap, expected)[0] == 4
        assert ref.inflate_one(stream, 10, 0)[0] == 4   # room is not what it lacks
    names = [m[0] for m in bi.malformed()]
    assert not set(names) & {d[0] for d in bi.deviations()}
    for want in ("dyn_16_first", "dyn_repeat_overruns", "dyn_no_end_of_block", "dyn_incomplete_lit", "dyn_incomplete_dist",
                 "dyn_oversubscribed_lit", "dyn_oversubscribed_dist", "dyn_incomplete_cl", "dyn_hlit_30", "dyn_hdist_30",
                 "dyn_length_without_dist_code", "dyn_one_dist_unused_code"):
        m = bi.malformed()[names.index(want)]
        assert m[2] == m[3] and m[4] == 4 and len(m[1]) < 400 and (m[1][2] >> 1) & 3 == 2, want


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
