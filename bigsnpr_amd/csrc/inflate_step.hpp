// inflate_step.hpp — the statement of one zlib stream (RFC 1950 around RFC 1951): what bsn_inflate and the BGEN entries
// make of the compressed probabilities of one variant (src/read-bgen.cpp:41-47 of the reference calls zlib's uncompress
// there).  Shared by the kernel (bgen.hip, k_inflate), the CPU statement (tests/native/inflate_ref.cpp) and the
// stand-alone sanitizer program (tests/native/inflate_fuzz.cpp): the three cannot drift apart.
//
// The decoder is written once, over a SINK that moves bytes: `Serial` below writes them one by one into the caller's
// buffer; the kernel's sink spreads a match over the lanes of a wave and keeps the 32-KiB window in LDS.  Every decision
// — what is read, whether a symbol, a length, a distance or a block is valid, whether the output still has room — is
// taken HERE, before the sink is asked to move anything; a sink checks nothing and needs to check nothing.
//
// Two properties hold by construction (DESIGN.md 3.5m gives the argument in full):
//   bounds       `in` is read only through Bits::need (in_pos < in_len is tested before every byte); a literal is put
//                only after pos < out_cap, a match only after dist <= pos and pos + len <= out_cap.
//   termination  every turn of every loop consumes at least one input bit or produces at least one output byte, so the
//                work is bounded by 8 * in_len + out_cap.
// Where this deviates from zlib 1.2.11 on malformed input it refuses: an incomplete literal/length set is an error even
// in the one-code case zlib lets pass.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BSN_INFLATE_HD __host__ __device__ __forceinline__
#else
#define BSN_INFLATE_HD inline
#endif

namespace bsn {
namespace inflate {

// status of one stream
constexpr int kOk = 0, kBadHeader = 1, kInputExhausted = 2, kOutputFull = 3, kInvalid = 4, kTooFarBack = 5, kBadAdler = 6,
              kWrongLength = 7;

constexpr int kMaxBits = 15, kMaxLit = 288, kMaxDist = 32, kWindow = 32768, kMaxMatch = 258;
constexpr uint32_t kAdlerMod = 65521;

// Work tables of one stream: canonical Huffman codes as "number of codes of each length" + "symbols in code order".
// On the device they sit in LDS.  The code-length code of a dynamic block lives in cnt_l / sym_l until the two real
// codes are built from `lens`.
struct Tables {
  uint16_t lens[kMaxLit + kMaxDist];
  uint16_t cnt_l[kMaxBits + 1], sym_l[kMaxLit];
  uint16_t cnt_d[kMaxBits + 1], sym_d[kMaxDist];
  uint16_t offs[kMaxBits + 1];
};

// ---- input: a bit reader that never reads past in_len ---------------------------------------------------------------------
struct Bits {
  const uint8_t *in;
  int64_t in_len, in_pos;
  uint32_t buf;
  int cnt;
  // at least n <= 16 bits in buf, or false: the input is exhausted
  BSN_INFLATE_HD bool need(int n) {
    while (cnt < n) {
      if (in_pos >= in_len) return false;
      buf |= (uint32_t)in[in_pos++] << cnt;
      cnt += 8;
    }
    return true;
  }
  BSN_INFLATE_HD uint32_t take(int n) {   // after need(n)
    const uint32_t v = buf & ((1u << n) - 1u);
    buf >>= n;
    cnt -= n;
    return v;
  }
};

// ---- canonical codes --------------------------------------------------------------------------------------------------------
// count / symbol from n code lengths.  0: complete (or no code at all); > 0: incomplete, that many codes of the longest
// length are unused; < 0: over-subscribed.
BSN_INFLATE_HD int build(uint16_t *count, uint16_t *symbol, uint16_t *offs, const uint16_t *length, int n) {
  for (int l = 0; l <= kMaxBits; l++) count[l] = 0;
  for (int s = 0; s < n; s++) count[length[s]]++;
  if (count[0] == n) return 0;
  int left = 1;
  for (int l = 1; l <= kMaxBits; l++) {
    left <<= 1;
    left -= count[l];
    if (left < 0) return left;
  }
  offs[1] = 0;
  for (int l = 1; l < kMaxBits; l++) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
  for (int s = 0; s < n; s++)
    if (length[s] != 0) symbol[offs[length[s]]++] = (uint16_t)s;
  return left;
}

// one symbol, bit by bit (each turn consumes a bit).  -1: no code of up to 15 bits matches; -2: input exhausted.
// index + (code - first) stays below the number of symbols that have a code, so the look-up is inside `symbol`.
BSN_INFLATE_HD int decode(Bits &b, const uint16_t *count, const uint16_t *symbol) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= kMaxBits; l++) {
    if (!b.need(1)) return -2;
    code |= (int)b.take(1);
    const int c = count[l];
    if (code - c < first) return symbol[index + (code - first)];
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

// ---- the serial sink ----------------------------------------------------------------------------------------------------------
// (the interface of a sink: lit, copy, after, finish; pos is the number of bytes produced before the call)
struct Serial {
  uint8_t *out;
  uint32_t a = 1, b = 0;   // Adler-32 of what has been produced
  BSN_INFLATE_HD explicit Serial(uint8_t *o) : out(o) {}
  BSN_INFLATE_HD void put(int64_t pos, uint8_t v) {
    out[pos] = v;
    a += v;
    if (a >= kAdlerMod) a -= kAdlerMod;
    b += a;
    if (b >= kAdlerMod) b -= kAdlerMod;
  }
  BSN_INFLATE_HD void lit(int64_t pos, uint8_t v) { put(pos, v); }
  // out[pos + i] = out[pos + i - dist], i ascending: for dist < len the run repeats with period dist
  BSN_INFLATE_HD void copy(int64_t pos, int dist, int len) {
    for (int i = 0; i < len; i++) put(pos + i, out[pos + i - dist]);
  }
  BSN_INFLATE_HD void after(int64_t) {}
  BSN_INFLATE_HD uint32_t finish(int64_t) { return (b << 16) | a; }
};

// ---- one stream ----------------------------------------------------------------------------------------------------------------
template <class Sink>
BSN_INFLATE_HD int stream(const uint8_t *in, int64_t in_len, int64_t out_cap, int64_t expected_len, Tables &t, Sink &sink) {
  // base value and number of extra bits of the length symbols 257 .. 285 and of the distance symbols 0 .. 29 (RFC 1951 3.2.5)
  constexpr uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  constexpr uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  constexpr uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  constexpr uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

  if (in_len < 2) return kInputExhausted;
  const uint32_t cmf = in[0], flg = in[1];
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return kBadHeader;

  Bits b{in, in_len, 2, 0u, 0};
  int64_t pos = 0;
  for (;;) {
    if (!b.need(3)) return kInputExhausted;
    const uint32_t last = b.take(1), type = b.take(2);
    if (type == 3) return kInvalid;
    if (type == 0) {
      // stored: the rest of the current byte is dropped, LEN and its complement, LEN bytes
      b.take(b.cnt & 7);
      if (!b.need(16)) return kInputExhausted;
      const uint32_t len = b.take(16);
      if (!b.need(16)) return kInputExhausted;
      const uint32_t nlen = b.take(16);
      if ((len ^ 0xFFFFu) != nlen) return kInvalid;
      for (uint32_t i = 0; i < len; i++) {
        if (!b.need(8)) return kInputExhausted;
        if (pos >= out_cap) return kOutputFull;
        sink.lit(pos, (uint8_t)b.take(8));
        pos++;
        sink.after(pos);
      }
    } else {
      if (type == 1) {
        for (int s = 0; s < 144; s++) t.lens[s] = 8;
        for (int s = 144; s < 256; s++) t.lens[s] = 9;
        for (int s = 256; s < 280; s++) t.lens[s] = 7;
        for (int s = 280; s < 288; s++) t.lens[s] = 8;
        build(t.cnt_l, t.sym_l, t.offs, t.lens, 288);
        // thirty codes of five bits: the two unused ones are the invalid distance symbols 30 and 31
        for (int s = 0; s < 30; s++) t.lens[s] = 5;
        build(t.cnt_d, t.sym_d, t.offs, t.lens, 30);
      } else {
        if (!b.need(14)) return kInputExhausted;
        const int nlen = (int)b.take(5) + 257, ndist = (int)b.take(5) + 1, ncode = (int)b.take(4) + 4;
        if (nlen > 286 || ndist > 30) return kInvalid;
        for (int i = 0; i < 19; i++) t.lens[i] = 0;
        for (int i = 0; i < ncode; i++) {
          if (!b.need(3)) return kInputExhausted;
          t.lens[order[i]] = (uint16_t)b.take(3);
        }
        if (build(t.cnt_l, t.sym_l, t.offs, t.lens, 19) != 0) return kInvalid;   // the code-length code must be complete
        int idx = 0;
        while (idx < nlen + ndist) {
          const int sym = decode(b, t.cnt_l, t.sym_l);
          if (sym < 0) return sym == -2 ? kInputExhausted : kInvalid;
          if (sym < 16) {
            t.lens[idx++] = (uint16_t)sym;
          } else {
            int rep, val = 0;
            if (sym == 16) {
              if (idx == 0) return kInvalid;   // nothing to repeat
              val = t.lens[idx - 1];
              if (!b.need(2)) return kInputExhausted;
              rep = 3 + (int)b.take(2);
            } else if (sym == 17) {
              if (!b.need(3)) return kInputExhausted;
              rep = 3 + (int)b.take(3);
            } else {
              if (!b.need(7)) return kInputExhausted;
              rep = 11 + (int)b.take(7);
            }
            if (idx + rep > nlen + ndist) return kInvalid;
            while (rep--) t.lens[idx++] = (uint16_t)val;
          }
        }
        if (t.lens[256] == 0) return kInvalid;   // no end-of-block code
        // build only reads `lens`: both codes are built from it in place.  An incomplete literal/length set is refused
        if (build(t.cnt_l, t.sym_l, t.offs, t.lens, nlen) != 0) return kInvalid;
        const int left = build(t.cnt_d, t.sym_d, t.offs, t.lens + nlen, ndist);
        // incomplete distance set: only the single code of one bit that zlib accepts
        if (left < 0 || (left > 0 && !(ndist - (int)t.cnt_d[0] == 1 && t.cnt_d[1] == 1))) return kInvalid;
      }
      for (;;) {
        int sym = decode(b, t.cnt_l, t.sym_l);
        if (sym < 0) return sym == -2 ? kInputExhausted : kInvalid;
        if (sym < 256) {
          if (pos >= out_cap) return kOutputFull;
          sink.lit(pos, (uint8_t)sym);
          pos++;
        } else if (sym == 256) {
          break;
        } else {
          sym -= 257;
          if (sym >= 29) return kInvalid;   // length symbols 286, 287
          if (!b.need(lext[sym])) return kInputExhausted;
          const int len = lbase[sym] + (int)b.take(lext[sym]);
          const int ds = decode(b, t.cnt_d, t.sym_d);
          if (ds < 0) return ds == -2 ? kInputExhausted : kInvalid;
          if (ds >= 30) return kInvalid;
          if (!b.need(dext[ds])) return kInputExhausted;
          const int dist = dbase[ds] + (int)b.take(dext[ds]);
          if ((int64_t)dist > pos) return kTooFarBack;
          if (pos + len > out_cap) return kOutputFull;
          sink.copy(pos, dist, len);
          pos += len;
        }
        sink.after(pos);
      }
    }
    if (last) break;
  }
  // trailer: Adler-32 of the output, most significant byte first, from the next byte boundary
  b.take(b.cnt & 7);
  uint32_t want = 0;
  for (int i = 0; i < 4; i++) {
    if (!b.need(8)) return kInputExhausted;
    want = (want << 8) | b.take(8);
  }
  if (sink.finish(pos) != want) return kBadAdler;
  if (pos != expected_len) return kWrongLength;
  return kOk;
}

// the statement in its plain form: one stream into the caller's buffer, byte by byte
BSN_INFLATE_HD int inflate_stream(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t expected_len) {
  Tables t;
  Serial sink(out);
  return stream(in, in_len, out_cap, expected_len, t, sink);
}

}  // namespace inflate
}  // namespace bsn
