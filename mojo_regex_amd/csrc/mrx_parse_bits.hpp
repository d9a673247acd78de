// Numbers (include/mrx.h, "numbers"): one piece of bytes parsed as a whole to an int64 or to the bits of a double.
// Host and device code: k_parse (mrx_parse.hip) calls parse_piece per lane, and tools/parse_check.cpp runs the same
// function on the CPU against strtoll, strtoull and strtod.
//
// A piece is read through gather_window, 16 bytes a step, so only the aligned 16-byte words that hold one of its bytes
// are loaded, and what those words hold outside the piece is masked to zero before a byte is classified.  The parse is
// a byte-at-a-time state machine; the window is only how the bytes arrive.
//
// Nothing wraps.  An integer's magnitude is kept in 64 bits with a sticky overflow flag.  A float's mantissa digits
// build d while d <= 2^53 and stop changing it afterwards (it stays above 2^53, which is what the verdict needs); zeros
// are held back and multiplied in only when a non-zero digit follows, so the zeros that end the mantissa never reach
// d: they are its factors of ten.  The exponent's magnitude stops growing at 10^9, far outside what can be answered
// and far inside an int64 next to the digit counts of a piece (a text has at most 2^31 bytes).
#pragma once
#include <cstdint>

#include "../../include/mrx.h"
#include "mrx_gather_bits.hpp"

namespace mrx {

constexpr uint64_t kParseMantissaMax = (uint64_t)1 << 53;   // integers up to here are doubles
constexpr int64_t kParseExpStop = 1000000000;

// 10^k for 0 <= k <= 22: the powers of ten that are doubles
MRX_HD double parse_pow10(int k) {
  constexpr double t[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                            1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  return t[k];
}

MRX_HD int parse_hex_digit(unsigned c) {   // 0..15, or -1
  if (c - '0' <= 9u) return (int)(c - '0');
  const unsigned l = c | 0x20;
  return l - 'a' <= 5u ? (int)(l - 'a') + 10 : -1;
}

// [+-]?[0-9]+ (hex = false) or [+-]?(0[xX])?[0-9a-fA-F]+ fed a byte at a time
struct ParseInt {
  enum { START, SIGNED, ZERO, PREFIX, DIGITS, BAD };   // ZERO: one '0' and nothing else, so an x may follow
  bool hex;
  int state = START;
  bool neg = false, over = false;
  uint64_t mag = 0;
  MRX_HD explicit ParseInt(bool hex_) : hex(hex_) {}
  MRX_HD void step(unsigned c) {
    if (state == BAD) return;
    if (state == START && (c == '+' || c == '-')) {
      neg = c == '-';
      state = SIGNED;
      return;
    }
    if (hex && state == ZERO && (c | 0x20) == 'x') {
      state = PREFIX;
      return;
    }
    const int d = hex ? parse_hex_digit(c) : c - '0' <= 9u ? (int)(c - '0') : -1;
    if (d < 0) {
      state = BAD;
      return;
    }
    const g_u128 t = (g_u128)mag * (hex ? 16u : 10u) + (unsigned)d;
    over |= (uint64_t)(t >> 64) != 0;
    mag = (uint64_t)t;
    state = (state == START || state == SIGNED) && d == 0 ? ZERO : DIGITS;
  }
  // 16 more decimal digits would change nothing: the magnitude has overflowed already
  MRX_HD bool past_digits() const { return state == DIGITS && over; }
  MRX_HD int finish(uint64_t* bits) const {
    if (state != ZERO && state != DIGITS) return MRX_NUM_MALFORMED;
    const uint64_t limit = ((uint64_t)1 << 63) - (neg ? 0 : 1);
    if (over || mag > limit) return MRX_NUM_RANGE;
    *bits = neg ? (uint64_t)0 - mag : mag;
    return MRX_NUM_OK;
  }
};

// [+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)? fed a byte at a time
struct ParseFloat {
  enum { START, SIGNED, INT, FRAC, EXP, EXP_SIGNED, EXP_DIGITS, BAD };
  int state = START;
  bool neg = false, exp_neg = false, any = false;   // any: the mantissa has a digit
  uint64_t d = 0;                                   // the mantissa's digits without the zeros held back
  int64_t zeros = 0, frac = 0, exp = 0;             // zeros held back, digits behind the point, |exponent|
  MRX_HD void digit(unsigned v) {
    any = true;
    if (state == FRAC) ++frac;
    if (v == 0) {
      ++zeros;
      return;
    }
    if (d == 0) zeros = 0;   // leading zeros
    for (; zeros > 0 && d <= kParseMantissaMax; --zeros) d *= 10;
    zeros = 0;
    if (d <= kParseMantissaMax) d = d * 10 + v;
  }
  MRX_HD void step(unsigned c) {
    const bool dig = c - '0' <= 9u;
    switch (state) {
      case START:
        if (c == '+' || c == '-') {
          neg = c == '-';
          state = SIGNED;
          return;
        }
        [[fallthrough]];
      case SIGNED:
        state = dig ? INT : c == '.' ? FRAC : BAD;
        if (dig) digit(c - '0');
        return;
      case INT:
      case FRAC:
        if (dig) {
          digit(c - '0');
        } else if (c == '.' && state == INT) {
          state = FRAC;
        } else if ((c | 0x20) == 'e' && any) {
          state = EXP;
        } else {
          state = BAD;
        }
        return;
      case EXP:
        if (c == '+' || c == '-') {
          exp_neg = c == '-';
          state = EXP_SIGNED;
          return;
        }
        [[fallthrough]];
      case EXP_SIGNED:
      case EXP_DIGITS:
        state = dig ? EXP_DIGITS : BAD;
        if (dig && exp < kParseExpStop) exp = exp * 10 + (int64_t)(c - '0');
        return;
      default:
        return;
    }
  }
  // 16 more mantissa digits would change nothing: d is above 2^53 for good, so neither q nor the zeros matter
  MRX_HD bool past_digits() const { return (state == INT || state == FRAC) && d > kParseMantissaMax; }
  MRX_HD int finish(uint64_t* bits) const {
    if (!(state == INT || (state == FRAC && any) || state == EXP_DIGITS)) return MRX_NUM_MALFORMED;
    double v = 0.0;
    if (d != 0) {
      const int64_t q = (exp_neg ? -exp : exp) - frac + zeros;   // the zeros held back are d's factors of ten
      if (d > kParseMantissaMax || q < -22 || q > 22) return MRX_NUM_RANGE;
      v = q >= 0 ? (double)d * parse_pow10((int)q) : (double)d / parse_pow10((int)-q);
    }
    union {
      double f;
      uint64_t u;
    } w;
    w.f = v;
    *bits = w.u | ((uint64_t)neg << 63);
    return MRX_NUM_OK;
  }
};

// are the 8 bytes of x all '0' .. '9'?  (high nibbles 3, and no low nibble carries into them when 6 is added)
MRX_HD bool parse_all_digits(uint64_t x) {
  const uint64_t hi = 0xF0F0F0F0F0F0F0F0ull, threes = 0x3030303030303030ull;
  return (x & hi) == threes && ((x + 0x0606060606060606ull) & hi) == threes;
}

// the bytes of a piece through a machine, 16 a window; non-zero = the machine has refused the piece.  A long run of
// digits behind the point where the verdict is RANGE already (a 500-digit field) is passed a window at a time: it
// still has to be read, since a byte outside the grammar further on makes the piece malformed.
template <class Machine>
MRX_HD int parse_feed(Machine& m, const uint8_t* p, int64_t len) {
  for (int64_t at = 0; at < len; at += 16) {
    const int take = len - at < 16 ? (int)(len - at) : 16;
    g_u128 w = gather_window(p + at, take);
    if (take < 16) w &= ((g_u128)1 << (8 * take)) - 1;
    uint64_t half = (uint64_t)w;
    if (take == 16 && m.past_digits() && parse_all_digits(half) && parse_all_digits((uint64_t)(w >> 64))) continue;
    for (int k = 0; k < take; ++k) {
      if (k == 8) half = (uint64_t)(w >> 64);
      m.step((unsigned)(half & 0xff));
      half >>= 8;
    }
    if (m.state == Machine::BAD) return MRX_NUM_MALFORMED;   // (the rest of the piece cannot mend it)
  }
  return MRX_NUM_OK;
}

// The piece p[0 .. len) under `kind` (MRX_NUM_INT10 / INT16 / FLOAT, checked by the caller): its status, and for
// MRX_NUM_OK the value's 64 bits in *bits (otherwise *bits is left alone).  Nothing is loaded for len <= 0.
MRX_HD int parse_piece(const uint8_t* p, int64_t len, int kind, uint64_t* bits) {
  if (len <= 0) return MRX_NUM_EMPTY;
  if (kind == MRX_NUM_FLOAT) {
    ParseFloat m;
    if (parse_feed(m, p, len)) return MRX_NUM_MALFORMED;
    return m.finish(bits);
  }
  ParseInt m(kind == MRX_NUM_INT16);
  if (parse_feed(m, p, len)) return MRX_NUM_MALFORMED;
  return m.finish(bits);
}

}  // namespace mrx
