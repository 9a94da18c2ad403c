"""Inputs of the BGEN tests (tests/test_inflate_cpu.py, tests/test_bgen_cpu.py, tests/test_gpu_bgen.py): a reader for
the R raw vectors that hold the reference's example .bgen / .bgi files (and for the matrix of its dosages), a writer of BGEN v1.2 files (layout 2, zlib,
8 bits) with their .bgi index, a small deflate emitter for stored, fixed-Huffman and dynamic-Huffman blocks from an
explicit list of literals and (length, distance) pairs — zlib itself never emits a distance above 32 506, a 15-bit code
on a few byte values or a one-code distance set, so the limits are hit on purpose with it —, the corpus of valid
streams, the fixed list of malformed ones, the one stream zlib accepts and the statement refuses, and the decode of a
file through Python's zlib that the device results are held against."""
import gzip
import os
import sqlite3
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DECODE_BYTES = (207 - np.floor(np.arange(511) * 100 / 255 + 0.5)).astype(np.uint8)   # no k * 100 / 255 is a tie
DECODE_DOSAGE = np.arange(510, -1, -1) / 255


# ---- R raw vectors ---------------------------------------------------------------------------------------------------------
def read_rds_raw(path):
    """the bytes of an .rds file that holds one raw vector: gzip, XDR serialisation ("X\\n", three version integers, for
    version 3 the native encoding), then one RAWSXP (type 24): its length and its bytes"""
    with gzip.open(path, "rb") as f:
        d = f.read()
    assert d[:2] == b"X\n", "not an XDR serialisation"
    version, = struct.unpack(">i", d[2:6])
    p = 14
    if version >= 3:
        n, = struct.unpack(">i", d[p:p + 4])
        p += 4 + n
    flags, n = struct.unpack(">ii", d[p:p + 8])
    assert flags & 0xFF == 24, "not a raw vector"
    assert len(d) >= p + 8 + n
    return d[p + 8:p + 8 + n]


def read_rds_doubles(path):
    """the values of an .rds file that holds one double vector or matrix (REALSXP, type 14; its attributes are not read)"""
    with gzip.open(path, "rb") as f:
        d = f.read()
    assert d[:2] == b"X\n", "not an XDR serialisation"
    version, = struct.unpack(">i", d[2:6])
    p = 14
    if version >= 3:
        n, = struct.unpack(">i", d[p:p + 4])
        p += 4 + n
    flags, n = struct.unpack(">ii", d[p:p + 8])
    assert flags & 0xFF == 14, "not a double vector"
    return np.frombuffer(d, dtype=">f8", count=n, offset=p + 8).astype(np.float64)


def example_files(tmp_dir):
    """the reference's example.bgen + example.bgen.bgi written to tmp_dir; returns the .bgen path"""
    bgen = os.path.join(str(tmp_dir), "example.bgen")
    with open(bgen, "wb") as f:
        f.write(read_rds_raw(os.path.join(GOLDEN, "bgen_example.rds")))
    with open(bgen + ".bgi", "wb") as f:
        f.write(read_rds_raw(os.path.join(GOLDEN, "bgi_example.rds")))
    return bgen


# ---- deflate emitter ---------------------------------------------------------------------------------------------------------
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
          8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)"""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        """a Huffman code of n bits, most significant first"""
        for i in range(n - 1, -1, -1):
            self.bits((v >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def _fixed_litlen(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def apply_tokens(tokens, start=b""):
    out = bytearray(start)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, dist = t
            for _ in range(ln):
                out.append(out[-dist])
    return bytes(out)


def fixed_block(w, tokens, last=True):
    """one fixed-Huffman block from literals (ints) and (length, distance) pairs; no check of the distances"""
    w.bits(1 if last else 0, 1)
    w.bits(1, 2)
    for t in tokens:
        if isinstance(t, int):
            _fixed_litlen(w, t)
        else:
            ln, dist = t
            s = 28 if ln == 258 else max(i for i in range(28) if _LBASE[i] <= ln)
            _fixed_litlen(w, 257 + s)
            w.bits(ln - _LBASE[s], _LEXT[s])
            d = max(i for i in range(30) if _DBASE[i] <= dist)
            w.code(d, 5)
            w.bits(dist - _DBASE[d], _DEXT[d])
    _fixed_litlen(w, 256)


def stored_block(w, data, last=True, nlen=None):
    w.bits(1 if last else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    w.out += data


def zlib_wrap(w, content):
    w.align()
    return b"\x78\x01" + bytes(w.out) + struct.pack(">I", zlib.adler32(content))


def emit(tokens):
    """a zlib stream of one fixed block from the tokens, and what it inflates to"""
    w = BitWriter()
    fixed_block(w, tokens)
    content = apply_tokens(tokens)
    return zlib_wrap(w, content), content


def token_spans(tokens, start=0):
    """[(pos, len, dist)] of the matches of a token list whose first byte is byte `start` of the output"""
    pos, out = start, []
    for t in tokens:
        if isinstance(t, int):
            pos += 1
        elif t[0] != "raw":
            out.append((pos, t[0], t[1]))
            pos += t[0]
    return out


def flush_spans(tokens, flush_bytes=2048):
    """[(flushed, pos)] of the flushes a sink takes that empties its pending bytes after every token of a Huffman block
    once `flush_bytes` or more are waiting (k_inflate's: kFlushBytes), the final one included"""
    pos, flushed, out = 0, 0, []
    for t in tokens:
        pos += 1 if isinstance(t, int) else t[0]
        if pos - flushed >= flush_bytes:
            out.append((flushed, pos))
            flushed = pos
    return out + [(flushed, pos)]


# ---- dynamic blocks ----------------------------------------------------------------------------------------------------------
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 10 + [5] * 6 + [4] * 3   # a complete code-length code: 13 codes of 4 bits, 6 of 5 (13 / 16 + 6 / 32 = 1)


def canonical(lens):
    """RFC 1951 3.2.2: {symbol: (code, bits)} of the symbols with a non-zero length.  Nothing is checked: an
    over-subscribed list gives codes that do not fit their length, an incomplete one leaves codes unused."""
    count = [0] * (max(list(lens) + [0]) + 2)
    for n in lens:
        if n:
            count[n] += 1
    code, nxt = 0, [0] * len(count)
    for n in range(1, len(count)):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def lens_of(d, n):
    """a list of n code lengths from {symbol: length}"""
    out = [0] * n
    for s, v in d.items():
        out[s] = v
    return out


def dynamic_block(w, tokens, lit_lens, dist_lens, last=True, cl_syms=None, cl_lens=None):
    """one dynamic-Huffman block.  lit_lens / dist_lens: the code lengths of the literal/length symbols 0 .. and of the
    distance symbols 0 .., whose counts go into HLIT / HDIST as they are.  cl_syms: the code lengths as (symbol, repeat)
    pairs of the code-length alphabet — (0 .. 15, 1) a length, (16, 3 .. 6) the previous one again, (17, 3 .. 10) and
    (18, 11 .. 138) zeros; default: every length as its own symbol.  cl_lens: the 19 lengths of the code-length code
    (default CL_LENS).  tokens: literals, (length, distance) pairs, (length, None) = the length symbol alone, ("raw", v, n)
    = n bits as they are; the end-of-block code follows them.  tokens=None: the header and the code lengths only.
    Nothing is checked and nothing raises: a symbol that has no code is left out."""
    cl_lens = CL_LENS if cl_lens is None else cl_lens
    if cl_syms is None:
        cl_syms = [(n, 1) for n in list(lit_lens) + list(dist_lens)]
    ncode = max([4] + [i + 1 for i in range(19) if cl_lens[_CL_ORDER[i]]])
    w.bits(1 if last else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257, 5)
    w.bits(len(dist_lens) - 1, 5)
    w.bits(ncode - 4, 4)
    for i in range(ncode):
        w.bits(cl_lens[_CL_ORDER[i]], 3)
    cl = canonical(cl_lens)
    for s, rep in cl_syms:
        if s in cl:
            w.code(*cl[s])
        if s == 16:
            w.bits(rep - 3, 2)
        elif s == 17:
            w.bits(rep - 3, 3)
        elif s == 18:
            w.bits(rep - 11, 7)
    if tokens is None:
        return
    lit, dst = canonical(lit_lens), canonical(dist_lens)

    def put(codes, s):
        if s in codes:
            w.code(*codes[s])

    for t in tokens:
        if isinstance(t, int):
            put(lit, t)
        elif t[0] == "raw":
            w.bits(t[1], t[2])
        else:
            ln, dist = t
            s = 28 if ln == 258 else max(i for i in range(28) if _LBASE[i] <= ln)
            put(lit, 257 + s)
            w.bits(ln - _LBASE[s], _LEXT[s])
            if dist is not None:
                d = max(i for i in range(30) if _DBASE[i] <= dist)
                put(dst, d)
                w.bits(dist - _DBASE[d], _DEXT[d])
    put(lit, 256)


def emit_dynamic(tokens, lit_lens, dist_lens, **kw):
    """a zlib stream of one dynamic block from the tokens, and what it inflates to"""
    w = BitWriter()
    dynamic_block(w, tokens, lit_lens, dist_lens, **kw)
    content = apply_tokens(tokens)
    return zlib_wrap(w, content), content


# ---- the corpus ------------------------------------------------------------------------------------------------------------------
def _data(n, seed=1):
    """compressible bytes: a few values, runs, and the odd repeat far back"""
    rng = np.random.default_rng(seed)
    a = rng.choice(np.array([0, 0, 0, 255, 1, 254, 17, 128], dtype=np.uint8), n)
    odd = rng.random(n) < 0.05
    a[odd] = rng.integers(0, 256, int(odd.sum()), dtype=np.uint8)
    return a.tobytes()


def _compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


SPECS = {}   # name -> what the stream was emitted from (tokens of the whole stream from byte 0, code lengths): the claims
             # of test_corpus_covers_what_it_claims are read off these, which corpus() has held against zlib


def _dynamic_and_ring_cases():
    """dynamic blocks that zlib's compressor does not produce, and matches and flushes at the edges of k_inflate's ring
    and flush sizes (32 768 and kFlushBytes = 2 048)"""
    out = []

    def add(name, pair, **spec):
        SPECS[name] = spec
        out.append((name,) + pair)

    # code lengths 1 .. 14 on fourteen byte values, 15 on one more and on the end of the block: a complete set
    vals = [0, 255, 1, 254, 17, 128, 7, 64, 200, 33, 99, 150, 222, 5]
    lit = lens_of(dict([(v, k + 1) for k, v in enumerate(vals)] + [(77, 15), (256, 15)]), 257)
    tokens = [(vals + [77])[(7 * k) % 15] for k in range(90)]
    add("dyn_lit15", emit_dynamic(tokens, lit, [0]), tokens=tokens, lit_lens=lit, dist_lens=[0])
    # the one incomplete set the statement accepts: a single distance code of one bit
    lit = lens_of({97: 2, 98: 2, 256: 2, 257: 2}, 258)
    tokens = [97, (3, 1), 98, (3, 1), 97, 98, (3, 1)]
    add("dyn_one_dist", emit_dynamic(tokens, lit, [1]), tokens=tokens, lit_lens=lit, dist_lens=[1])
    # ... on distance symbol 29 with 286 + 30 lengths: both counts at their limits, 13 extra bits
    lit = [9] * 256 + [2] + [0] * 28 + [2]
    tokens = list(_data(32768, 12)) + [(258, 32768), (258, 24577)]
    add("dyn_one_dist_29", emit_dynamic(tokens, lit, [0] * 29 + [1]), tokens=tokens, lit_lens=lit, dist_lens=[0] * 29 + [1])
    # a run of symbol 16 that starts in the literal/length lengths and ends in the distance lengths
    lit, dist = [1] + [0] * 255 + [2, 2], [2, 2, 2, 2]
    cl_syms = [(1, 1), (18, 138), (18, 117), (2, 1), (16, 5)]
    tokens = [0, (3, 1), 0, 0, (3, 2), 0, (3, 3), 0, (3, 4)]
    add("dyn_run_crosses", emit_dynamic(tokens, lit, dist, cl_syms=cl_syms), tokens=tokens, lit_lens=lit, dist_lens=dist,
        cl_syms=cl_syms)
    # two dynamic blocks with different code sets; the second one's first match reaches into the bytes of the first
    lit1 = lens_of(dict([(v, 4) for v in range(0x61, 0x69)] + [(256, 3), (257, 3), (258, 2)]), 259)
    t1 = list(b"abcdefgh") + [(4, 3)] + list(b"hgfedcba") + [(3, 1), (4, 4)] + list(b"abcabcabhhgg") + [(4, 2), (3, 4)]
    lit2 = lens_of({0x30: 3, 0x31: 3, 0x32: 3, 0x33: 3, 256: 2, 264: 3, 285: 3}, 286)
    dist2 = [0] * 6 + [3] * 8
    n1 = len(apply_tokens(t1))
    t2 = [(10, n1 - 5), 0x30, 0x31, 0x32, 0x33, (258, 9), 0x33, (10, 100)]
    w = BitWriter()
    dynamic_block(w, t1, lit1, [2, 2, 2, 2], last=False)
    dynamic_block(w, t2, lit2, dist2, last=True)
    content = apply_tokens(t1 + t2)
    add("dyn_two_tables", (zlib_wrap(w, content), content), tokens=t1 + t2, first_block_bytes=n1, lit_lens=lit1,
        lit_lens2=lit2)
    # a match whose destination straddles the end of the ring
    tokens = list(_data(32700, 13)) + [(258, 50), 7]
    add("ring_end_dest", emit(tokens), tokens=tokens)
    # ... whose source straddles 32 768 while its destination straddles 65 536
    tokens = (list(_data(32768, 14)) + [(258, 30000 + 17 * i) for i in range(100)] + list(_data(6838, 15))
              + [(258, 32768), 9])
    add("ring_end_both", emit(tokens), tokens=tokens)
    # the largest flush, 2 047 + 258 bytes, and then one of exactly 2 048 that a match completes
    tokens = list(_data(2047, 16)) + [(258, 2047)] + list(_data(1790, 17)) + [(258, 100), 1, 2, 3]
    add("flush_2305", emit(tokens), tokens=tokens)
    # i % dist over all five passes of the 64 lanes
    tokens = list(_data(300, 18)) + [(258, 63), 5, (258, 65), 6, (258, 129), 7, (258, 257)]
    add("periodic_258", emit(tokens), tokens=tokens)
    # both Adler sums near 65 521 for the whole stream
    tokens = [255] + [(258, 1)] * 271
    add("adler_ff", emit(tokens), tokens=tokens)
    return out


_corpus = None


def corpus():
    """[(name, stream, content)]: valid streams, each checked here against zlib.decompress"""
    global _corpus
    if _corpus is not None:
        return _corpus
    big = _data(70000, 3)
    out = []
    for lv in (0, 1, 6, 9):
        out.append(("level%d" % lv, _compress(_data(5000, lv + 10), lv), _data(5000, lv + 10)))
    out.append(("fixed", _compress(_data(3000, 5), 6, zlib.Z_FIXED), _data(3000, 5)))
    out.append(("full_flush", _compress(_data(4001, 6), 6, flush_at=1237), _data(4001, 6)))
    out.append(("two_stored_blocks", _compress(big, 0), big))
    out.append(("level6_70000", _compress(big, 6), big))
    for n in (1, 13, 63, 64, 65):
        out.append(("bytes%d" % n, _compress(_data(n, n), 6), _data(n, n)))
    out.append(("empty", _compress(b"", 6), b""))
    lits = list(_data(40, 8))
    out.append(("len258_len3",) + emit(lits + [(258, 40), (3, 7), 5, (258, 1), 9]))
    out.append(("dist1_len258",) + emit([77, (258, 1), (258, 1), 3]))
    out.append(("periodic",) + emit(lits[:7] + [(200, 7), (100, 3), (64, 2), (65, 64), (63, 65)]))
    first = list(_data(32768, 9))
    out.append(("dist32768",) + emit(first + [(258, 32768), 1, (17, 32768), (5, 24577), (9, 24576)]))
    out.append(("dist_13_extra_bits",) + emit(first[:30000] + [(100, 24577 + 4000), (30, 16385 + 8191)]))
    # a stored block, then fixed blocks whose matches reach back into it and across the block boundary
    w = BitWriter()
    start = _data(300, 11)
    stored_block(w, start, last=False)
    fixed_block(w, [1, 2, (50, 300), (258, 2)], last=False)
    w.bits(0, 1); w.bits(0, 2); w.align(); w.bits(0, 16); w.bits(0xFFFF, 16)   # an empty stored block
    fixed_block(w, [(20, 100), 7], last=True)
    content = apply_tokens([7], apply_tokens([(20, 100)], apply_tokens([1, 2, (50, 300), (258, 2)], start)))
    out.append(("stored_then_fixed", zlib_wrap(w, content), content))
    out += _dynamic_and_ring_cases()
    assert max(len(c[2]) for c in out) <= 70000
    for name, s, c in out:
        assert zlib.decompress(s) == c, name
    _corpus = out
    return out


_malformed = None


def malformed():
    """[(name, stream, out_cap, expected_len, status)]: the fixed list of streams that must be refused, each with the
    status the statement gives it"""
    global _malformed
    if _malformed is not None:
        return _malformed
    data = _data(2000, 21)
    good = _compress(data, 6)
    n = len(data)
    out = []
    for cut in list(range(64)) + [len(good) - 1]:
        out.append(("truncated_%d" % cut, good[:cut], n, n, 2))
    bad = bytearray(good); bad[-2] ^= 0x10
    out.append(("adler", bytes(bad), n, n, 6))
    out.append(("expected_len_short", good, n, n - 1, 7))
    out.append(("expected_len_long", good, n + 1, n + 1, 7))
    out.append(("out_cap_one_short", good, n - 1, n - 1, 3))
    w = BitWriter(); stored_block(w, b"abcdef", nlen=0x1234)
    out.append(("bad_nlen", zlib_wrap(w, b"abcdef"), 6, 6, 4))
    # dynamic block whose code-length code is over-subscribed: 19 lengths of 1
    w = BitWriter(); w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)
    out.append(("oversubscribed", zlib_wrap(w, b""), 10, 10, 4))
    out.append(("distance_before_start", emit([1, 2, 3])[0][:2] + _bad_distance(), 20, 20, 5))
    w = BitWriter(); w.bits(1, 1); w.bits(3, 2)
    out.append(("block_type_3", zlib_wrap(w, b""), 4, 4, 4))
    out.append(("bad_header_cm", b"\x79\x01" + good[2:], n, n, 1))
    out.append(("bad_header_fcheck", b"\x78\x02" + good[2:], n, n, 1))
    out.append(("bad_header_fdict", b"\x78\x20" + good[2:], n, n, 1))
    w = BitWriter(); w.bits(1, 1); w.bits(1, 2); _fixed_litlen(w, 65); _fixed_litlen(w, 286)
    out.append(("length_symbol_286", zlib_wrap(w, b"A"), 300, 300, 4))
    w = BitWriter(); w.bits(1, 1); w.bits(1, 2); _fixed_litlen(w, 65); _fixed_litlen(w, 257); w.code(30, 5)
    out.append(("distance_symbol_30", zlib_wrap(w, b"A"), 300, 300, 4))
    out += [(name, s, 10, 10, 4) for name, s in _malformed_dynamic()]
    for name, s, cap, exp, status in out:
        if status != 7:   # zlib refuses them too (a wrong expected length is the caller's business)
            try:
                ok = len(zlib.decompress(s)) <= cap
            except zlib.error:
                ok = False
            assert not ok, name
    _malformed = out
    return out


def _malformed_dynamic():
    """[(name, stream)]: dynamic blocks that zlib and the statement (status 4) both refuse.  Where the fault is in the
    header or in the code lengths, the stream stops there; the four trailer bytes leave enough bits for a symbol that
    matches no code to be read to its end."""
    ok_lit = lens_of({97: 1, 256: 2, 257: 2}, 258)
    cases = [
        ("dyn_16_first", dict(tokens=None, lit_lens=ok_lit, dist_lens=[1], cl_syms=[(16, 3)])),
        ("dyn_repeat_overruns", dict(tokens=None, lit_lens=ok_lit[:257], dist_lens=[1], cl_syms=[(18, 138), (18, 138)])),
        ("dyn_no_end_of_block", dict(tokens=None, lit_lens=lens_of({97: 1, 98: 1}, 257), dist_lens=[0])),
        ("dyn_incomplete_lit", dict(tokens=None, lit_lens=lens_of({97: 2, 256: 2}, 257), dist_lens=[0])),
        ("dyn_incomplete_dist", dict(tokens=None, lit_lens=ok_lit, dist_lens=[2, 2])),
        ("dyn_oversubscribed_lit", dict(tokens=None, lit_lens=lens_of({97: 1, 98: 1, 256: 1}, 257), dist_lens=[0])),
        ("dyn_oversubscribed_dist", dict(tokens=None, lit_lens=ok_lit, dist_lens=[1, 1, 1])),
        ("dyn_incomplete_cl", dict(tokens=None, lit_lens=ok_lit, dist_lens=[1], cl_syms=[], cl_lens=lens_of({0: 1, 18: 2}, 19))),
        ("dyn_hlit_30", dict(tokens=None, lit_lens=lens_of({97: 1, 256: 1}, 287), dist_lens=[0], cl_syms=[])),
        ("dyn_hdist_30", dict(tokens=None, lit_lens=ok_lit, dist_lens=[0] * 30 + [1], cl_syms=[])),
        ("dyn_length_without_dist_code", dict(tokens=[97, (3, None)], lit_lens=ok_lit, dist_lens=[0])),
        ("dyn_one_dist_unused_code", dict(tokens=[97, (3, None), ("raw", 1, 1)], lit_lens=ok_lit, dist_lens=[1])),
    ]
    out = []
    for name, kw in cases:
        w = BitWriter()
        dynamic_block(w, kw.pop("tokens"), kw.pop("lit_lens"), kw.pop("dist_lens"), **kw)
        out.append((name, zlib_wrap(w, b"")))
    return out


def deviations():
    """[(name, stream, out_cap, expected_len, status)]: what zlib accepts and the statement refuses (inflate_step.hpp,
    DESIGN.md 3.5m) — a literal/length set that holds only the end-of-block code, at one bit.  zlib gives b"" for it."""
    w = BitWriter()
    dynamic_block(w, [], [0] * 256 + [1], [0])
    s = zlib_wrap(w, b"")
    assert zlib.decompress(s) == b""
    return [("dyn_only_end_of_block", s, 0, 0, 4)]


def _bad_distance():
    w = BitWriter()
    fixed_block(w, [1, 2, 3, (4, 4)])
    w.align()
    return bytes(w.out) + struct.pack(">I", 0)


def pack(streams, lens):
    """(in, in_off, out_off) of bsn_inflate / the twin for a list of streams and their output lengths"""
    in_off = np.zeros(len(streams) + 1, dtype=np.int64)
    in_off[1:] = np.cumsum([len(s) for s in streams])
    out_off = np.zeros(len(streams) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(lens)
    return np.frombuffer(b"".join(streams) + b"\0", dtype=np.uint8).copy(), in_off, out_off


# ---- BGEN writer -------------------------------------------------------------------------------------------------------------
def probabilities(N, K, seed=0, missing=0.01, confident=0.5):
    """(p0, p1, miss): N x K bytes with p0 + p1 <= 255 and a share of missing samples"""
    rng = np.random.default_rng(seed)
    p0 = rng.integers(0, 256, (N, K))
    p1 = (rng.random((N, K)) * (256 - p0)).astype(np.int64)
    sure = rng.random((N, K)) < confident
    call = rng.integers(0, 3, (N, K))
    p0 = np.where(sure, np.where(call == 0, 255, 0), p0)
    p1 = np.where(sure, np.where(call == 1, 255, 0), p1)
    miss = rng.random((N, K)) < missing
    return p0.astype(np.uint8), p1.astype(np.uint8), miss


def inflated_block(p0, p1, miss):
    """the 10 + 3 N bytes of one variant before compression"""
    N = p0.size
    pl = np.where(miss, 0x82, 2).astype(np.uint8)
    pr = np.empty(2 * N, dtype=np.uint8)
    pr[0::2], pr[1::2] = np.where(miss, 0, p0), np.where(miss, 0, p1)
    return struct.pack("<IHBB", N, 2, 2, 2) + pl.tobytes() + b"\x00\x08" + pr.tobytes()


def _lstr(s, fmt):
    b = s.encode()
    return struct.pack(fmt, len(b)) + b


def write_bgen(path, p0, p1, miss, compress=None, chrom="01", pos0=1000, flags=1 | (2 << 2), magic=b"bgen", pos=None,
               alleles=2, D_add=0, streams=None):
    """a BGEN v1.2 file of the N x K probabilities with its .bgi index; compress(j, block) -> zlib stream (default:
    zlib level 6); streams: ready-made streams by variant.  Returns the list of variant dicts (offset, id, alleles ...)"""
    N, K = p0.shape
    free = b""
    head = struct.pack("<III", 20 + len(free), K, N) + magic + free + struct.pack("<I", flags)
    body = bytearray(struct.pack("<I", len(head)) + head)
    variants = []
    for j in range(K):
        off = len(body)
        block = inflated_block(p0[:, j], p1[:, j], miss[:, j])
        if streams is not None and streams.get(j) is not None:
            z = streams[j]
        else:
            z = compress(j, block) if compress else zlib.compress(block, 6)
        a1, a2 = "ACGT"[j % 4], "CGTA"[j % 4]
        ps = pos0 + 7 * j if pos is None else pos
        rec = _lstr("id%d" % j, "<H") + _lstr("rs%d" % j, "<H") + _lstr(chrom, "<H") + struct.pack("<IH", ps, alleles)
        rec += _lstr(a1, "<I") + _lstr(a2, "<I")
        rec += struct.pack("<II", len(z) + 4, len(block) + D_add) + z
        body += rec
        variants.append(dict(chromosome=chrom, position=ps, rsid="rs%d" % j, allele1=a1, allele2=a2, offset=off,
                             size=len(rec), id="id%d" % j, snp_id="%s_%d_%s_%s" % (chrom.lstrip("0") or "0", ps, a1, a2)))
    with open(path, "wb") as f:
        f.write(body)
    if os.path.exists(path + ".bgi"):
        os.remove(path + ".bgi")
    db = sqlite3.connect(path + ".bgi")
    db.execute("CREATE TABLE Variant (chromosome TEXT NOT NULL, position INT NOT NULL, rsid TEXT NOT NULL, "
               "number_of_alleles INT NOT NULL, allele1 TEXT NOT NULL, allele2 TEXT NULL, file_start_position INT NOT NULL, "
               "size_in_bytes INT NOT NULL, PRIMARY KEY (chromosome, position, rsid, allele1, allele2, file_start_position)) "
               "WITHOUT ROWID")
    db.executemany("INSERT INTO Variant VALUES (?, ?, ?, 2, ?, ?, ?, ?)",
                   [(v["chromosome"], v["position"], v["rsid"], v["allele1"], v["allele2"], v["offset"], v["size"])
                    for v in variants])
    db.commit()
    db.close()
    return variants


# ---- a file through Python's zlib ------------------------------------------------------------------------------------------------
def parse_variant(raw, off):
    """(id, p0, p1, miss) of the record at `off` of the file bytes `raw`"""
    q = off
    strs = []
    for _ in range(3):
        n, = struct.unpack_from("<H", raw, q)
        strs.append(raw[q + 2:q + 2 + n].decode())
        q += 2 + n
    q += 6
    for _ in range(2):
        n, = struct.unpack_from("<I", raw, q)
        q += 4 + n
    C, D = struct.unpack_from("<II", raw, q)
    block = np.frombuffer(zlib.decompress(raw[q + 8:q + 4 + C]), dtype=np.uint8)
    assert block.size == D
    N = (D - 10) // 3
    pr = block[10 + N:]
    return strs[0], pr[0::2].astype(np.int64), pr[1::2].astype(np.int64), block[8:8 + N] >= 0x80


def decode_file(path, offsets, ind_row=None):
    """what the reference makes of the variants at `offsets`: FBM bytes (n x K, 3 = missing), dosages (NaN = missing),
    ids, and the three integer sums (nona, af, num) per variant"""
    raw = open(path, "rb").read()
    cols, dos, ids, sums = [], [], [], []
    for off in offsets:
        vid, p0, p1, miss = parse_variant(raw, int(off))
        if ind_row is not None:
            p0, p1, miss = p0[ind_row], p1[ind_row], miss[ind_row]
        k = 2 * p0 + p1
        cols.append(np.where(miss, 3, DECODE_BYTES[k]).astype(np.uint8))
        dos.append(np.where(miss, np.nan, DECODE_DOSAGE[k]))
        ids.append(vid)
        ok = ~miss
        sums.append((int(ok.sum()), int(k[ok].sum()), int((255 * (4 * p0 + p1) - k * k)[ok].sum())))
    return (np.asfortranarray(np.stack(cols, axis=1)), np.stack(dos, axis=1), ids, np.array(sums, dtype=np.int64))


def info_freq(sums):
    """src/read-bgen.cpp:72-75 in numpy doubles, operation by operation"""
    nona, af, num = (sums[:, k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        coef = 255 * (2 * nona)
        info = 1 - num * 2 * nona / (af * (coef - af))
        freq = 1 - af / coef
    return info, freq
