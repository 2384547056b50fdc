// TEST INFRASTRUCTURE: the emulator's stand-in for sortmerna_amd/csrc/smr_h16_ops.hpp (found first: -I tests/emu/shim comes first).
// Scalar host code on f16 BIT PATTERNS: every operation decodes its operands (exactly), computes in double (the sum of two f16 values is
// exact there: 40 binades + 11 bits < 53) and encodes the result with ONE rounding to nearest even -- what v_pk_add_f16 does.  The
// conversion is general (subnormals, overflow to infinity, NaN), so a value the kernel's exactness argument does not cover would come
// back rounded and show as a difference from the integer kernel.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

namespace smr {

inline double h16_decode_slow(uint16_t h) {
  const int s = h >> 15, e = (h >> 10) & 31, f = h & 1023;
  double v;
  if (e == 0) v = ldexp((double)f, -24);
  else if (e == 31) v = f ? NAN : INFINITY;
  else v = ldexp((double)(1024 + f), e - 25);
  return s ? -v : v;
}
inline double h16_decode(uint16_t h) {          // (all 65536 patterns, decoded once)
  static const double* const table = [] { double* t = new double[65536]; for (uint32_t i = 0; i < 65536u; i++) t[i] = h16_decode_slow((uint16_t)i); return t; }();
  return table[h];
}
inline uint16_t h16_encode(double v) {          // round to nearest, ties to even; on the bits of the double
  uint64_t b;
  memcpy(&b, &v, 8);
  const uint16_t s = (uint16_t)((b >> 63) << 15);
  const int be = (int)((b >> 52) & 0x7FF);
  uint64_t mant = b & ((1ull << 52) - 1);
  if (be == 0x7FF) return mant ? 0x7E00 : (uint16_t)(s | 0x7C00);
  if (be == 0) return s;                        // (zero, or a subnormal double: far below half of f16's smallest step)
  mant |= 1ull << 52;
  const int ex = be - 1023;                     // |v| = mant 2^(ex - 52), 2^52 <= mant < 2^53
  int q = ex - 10;                              // the unit of an 11-bit significand
  if (q < -24) q = -24;                         // subnormal range: the unit stays 2^-24
  const int sh = 52 + q - ex;                   // |v| / 2^q = mant / 2^sh, sh >= 42
  uint64_t r = 0;
  if (sh <= 63) {
    r = mant >> sh;
    const uint64_t rem = mant & ((1ull << sh) - 1), half = 1ull << (sh - 1);
    if (rem > half || (rem == half && (r & 1))) r++;
  }
  if (r == 0) return s;
  if (r == 2048) { r = 1024; q++; }
  if (r < 1024) return (uint16_t)(s | r);       // subnormal (q = -24)
  const int e = q + 25;
  if (e >= 31) return (uint16_t)(s | 0x7C00);   // (rounds to infinity from 65520 on)
  return (uint16_t)(s | (e << 10) | (r - 1024));
}

struct h16x2 { uint16_t lo, hi; };
inline h16x2 h2_from(uint32_t v) { h16x2 r; r.lo = (uint16_t)(v & 0xFFFF); r.hi = (uint16_t)(v >> 16); return r; }
inline uint32_t h2_bits(h16x2 v) { return (uint32_t)v.lo | ((uint32_t)v.hi << 16); }
inline uint32_t h16_of_int(int v) { return h16_encode((double)v); }
inline int h16_to_int(uint32_t half) { return (int)h16_decode((uint16_t)half); }
inline h16x2 h2_splat(int v) { return h2_from(h16_of_int(v) * 0x00010001u); }
inline h16x2 h2_add(h16x2 a, h16x2 b) { h16x2 r; r.lo = h16_encode(h16_decode(a.lo) + h16_decode(b.lo)); r.hi = h16_encode(h16_decode(a.hi) + h16_decode(b.hi)); return r; }
inline h16x2 h2_sub(h16x2 a, h16x2 b) { h16x2 r; r.lo = h16_encode(h16_decode(a.lo) - h16_decode(b.lo)); r.hi = h16_encode(h16_decode(a.hi) - h16_decode(b.hi)); return r; }
// v_pk_maximum3_f16: IEEE-754 maximum (a NaN operand gives NaN, +0 > -0), the result is one of the operands' patterns
inline uint16_t h16_maximum(uint16_t a, uint16_t b) {
  const double x = h16_decode(a), y = h16_decode(b);
  if (x != x || y != y) return 0x7E00;
  if (x == y) return (a & 0x8000) ? b : a;
  return x > y ? a : b;
}
inline h16x2 h2_max3(h16x2 a, h16x2 b, h16x2 c) { h16x2 r; r.lo = h16_maximum(h16_maximum(a.lo, b.lo), c.lo); r.hi = h16_maximum(h16_maximum(a.hi, b.hi), c.hi); return r; }
inline h16x2 h2_max(h16x2 a, h16x2 b) { return h2_max3(a, b, b); }

}  // namespace smr
