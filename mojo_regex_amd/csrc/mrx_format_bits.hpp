// Format (include/mrx.h, "format"): one cell of a number column written as text -- the inverse of mrx_parse_bits.hpp --
// and the assembly of a record from a template's segments, a lane per 16-byte block of the packed records.  Host and
// device code: k_format_sizes and k_format_gather (mrx_format.hip) call it per lane, mrx_testing_format_one and
// tools/format_check.cpp run the same functions on the CPU against Python's and C's printf.
//
// A cell is described once, by format_cell in the sizes kernel: a 64-bit WORD and a 32-bit DESCRIPTOR.
//   text cell     word = the address of its first byte, descriptor = its length (>= 0)
//   number cell   word = the unsigned magnitude (for MRX_COL_FIXED the scaled, rounded N), descriptor = kFmtNumber |
//                 length | sign << 5 | digits << 8 | digits behind the point << 16 | hex << 20
//   nothing       descriptor 0 (a status byte that is not MRX_NUM_OK, a RANGE verdict): an empty cell
// The gather never decides anything about a number again: it renders `digits` digits of the magnitude (zeros in front
// included) and places the bytes it was asked for.  No floating-point operation anywhere: MRX_COL_FIXED scales the
// double's 53-bit mantissa by 10^P in 128 bits, shifts by the binary exponent and rounds on the remainder, ties to even.
//
// The digits come without a division by a variable: the magnitude is cut into chunks of 8 decimal digits by constant
// divisors (multiply-high), and a chunk becomes 8 ASCII bytes by SWAR arithmetic; hex is a nibble spread.
#pragma once
#include <cstdint>

#include "../../include/mrx.h"
#include "mrx_expand_bits.hpp"
#include "mrx_gather_bits.hpp"

namespace mrx {

constexpr uint32_t kFmtNumber = 0x80000000u;            // descriptor: a number cell (a text's length has the bit clear)
constexpr uint64_t kFmtLimit = 10000000000000000000ull;   // 10^19: a FIXED cell's N stays below it
constexpr int kFmtCellMax = 21;                          // the longest number cell: a sign and 20 digits

MRX_HD uint64_t format_pow10(int k) {   // 10^k for 0 <= k <= 19
  constexpr uint64_t t[20] = {1ull,
                              10ull,
                              100ull,
                              1000ull,
                              10000ull,
                              100000ull,
                              1000000ull,
                              10000000ull,
                              100000000ull,
                              1000000000ull,
                              10000000000ull,
                              100000000000ull,
                              1000000000000ull,
                              10000000000000ull,
                              100000000000000ull,
                              1000000000000000ull,
                              10000000000000000ull,
                              100000000000000000ull,
                              1000000000000000000ull,
                              10000000000000000000ull};
  return t[k];
}

// decimal digits of v (1 for 0): the bit length gives the count to within one, a comparison settles it
MRX_HD int format_dec_digits(uint64_t v) {
  if (v == 0) return 1;
  const int bits = 64 - __builtin_clzll(v);
  const int d = (bits * 1233) >> 12;   // floor(bits * log10(2)), exact for bits <= 64
  return d + (d < 20 && v >= format_pow10(d) ? 1 : 0);
}
MRX_HD int format_hex_digits(uint64_t v) { return v == 0 ? 1 : (64 - __builtin_clzll(v) + 3) >> 2; }

// v < 10^8 as 8 ASCII digits, the most significant one in the lowest byte (memory order = reading order)
MRX_HD uint64_t format_dec8(uint32_t v) {
  const uint64_t x = (uint64_t)(v / 10000u) | ((uint64_t)(v % 10000u) << 32);   // two halves below 10^4
  const uint64_t q100 = ((x * 5243u) >> 19) & 0x0000007F0000007Full;               // each / 100 ...
  const uint64_t y = q100 | ((x - 100u * q100) << 16);                             // ... and % 100: four lanes below 100
  const uint64_t q10 = ((y * 103u) >> 10) & 0x000F000F000F000Full;
  return (q10 | ((y - 10u * q10) << 8)) + 0x3030303030303030ull;
}
// v as 8 lower-case hex digits, the most significant one in the lowest byte
MRX_HD uint64_t format_hex8(uint32_t v) {
  uint64_t t = v;
  t = (t | (t << 16)) & 0x0000FFFF0000FFFFull;
  t = (t | (t << 8)) & 0x00FF00FF00FF00FFull;
  t = (t | (t << 4)) & 0x0F0F0F0F0F0F0F0Full;   // nibble k in byte k
  t = __builtin_bswap64(t);
  const uint64_t above9 = ((t + 0x0606060606060606ull) >> 4) & 0x0101010101010101ull;
  return t + 0x3030303030303030ull + above9 * 39u;
}

// the magnitude as 24 digits, zeros in front: bytes 0..7 in c[0], 8..15 in c[1], 16..23 (the last digits) in c[2]
struct FormatDigits {
  uint64_t c0, c1, c2;
};
MRX_HD FormatDigits format_digits(uint64_t mag, bool hex) {
  FormatDigits d;
  if (hex) {
    d.c0 = 0x3030303030303030ull;
    d.c1 = format_hex8((uint32_t)(mag >> 32));
    d.c2 = format_hex8((uint32_t)mag);
  } else if (mag < 100000000ull) {   // counts, ids, cents: one chunk, and no 64-bit division
    d.c0 = d.c1 = 0x3030303030303030ull;
    d.c2 = format_dec8((uint32_t)mag);
  } else {
    const uint64_t top = mag / 10000000000000000ull, rest = mag % 10000000000000000ull;   // top < 1845
    d.c0 = format_dec8((uint32_t)top);
    d.c1 = format_dec8((uint32_t)(rest / 100000000ull));
    d.c2 = format_dec8((uint32_t)(rest % 100000000ull));
  }
  return d;
}
// bytes from .. from + 16 of those 24 (0 <= from < 24; zero behind the last one)
MRX_HD g_u128 format_digits_window(const FormatDigits& d, int from) {
  const int w = from >> 3, sh = 8 * (from & 7);
  const uint64_t a = w == 0 ? d.c0 : w == 1 ? d.c1 : d.c2;
  const uint64_t b = w == 0 ? d.c1 : w == 1 ? d.c2 : 0;
  const uint64_t c = w == 0 ? d.c2 : 0;
  const uint64_t lo = sh ? (a >> sh) | (b << (64 - sh)) : a;
  const uint64_t hi = sh ? (b >> sh) | (c << (64 - sh)) : b;
  return ((g_u128)hi << 64) | lo;
}

MRX_HD int format_desc_len(int32_t desc) { return desc >= 0 ? desc : desc & 31; }
MRX_HD int32_t format_number_desc(bool neg, int digits, int point, bool hex) {
  const int len = (neg ? 1 : 0) + digits + (point > 0 ? 1 : 0);
  return (int32_t)(kFmtNumber | (uint32_t)len | ((uint32_t)neg << 5) | ((uint32_t)digits << 8) | ((uint32_t)point << 16) |
                   ((uint32_t)hex << 20));
}

// MRX_COL_FIXED: N = round_half_even(|v| * 10^P) from the bits of a double, or false when it is not below 10^19
// (NaN and the infinities among them).  |v| = m * 2^e with m < 2^53; m * 10^P < 2^83.
MRX_HD bool format_fixed_scale(uint64_t bits, int P, uint64_t* N) {
  const int E = (int)((bits >> 52) & 0x7ff);
  const uint64_t frac = bits & (((uint64_t)1 << 52) - 1);
  if (E == 0x7ff) return false;
  const uint64_t m = E ? frac | ((uint64_t)1 << 52) : frac;
  const int e = E ? E - 1075 : -1074;
  const g_u128 prod = (g_u128)m * format_pow10(P);
  g_u128 q;
  if (e >= 0) {
    if (prod == 0) {
      q = 0;
    } else {
      if (e >= 64 || (prod >> (64 - e)) != 0) return false;   // 2^64 and more
      q = prod << e;
    }
  } else {
    const int s = -e;
    if (s >= 128) {
      q = 0;
    } else {
      q = prod >> s;
      const g_u128 half = (g_u128)1 << (s - 1), rem = prod & ((half << 1) - 1);
      if (rem > half || (rem == half && ((uint64_t)q & 1))) ++q;
    }
  }
  if ((uint64_t)(q >> 64) != 0 || (uint64_t)q >= kFmtLimit) return false;
  *N = (uint64_t)q;
  return true;
}

// One number cell (kind and arg checked by the caller): MRX_NUM_OK with the magnitude and the descriptor, or
// MRX_NUM_RANGE.  value: the int64, or the bits of the double.
MRX_HD int format_cell(int kind, int arg, uint64_t value, uint64_t* mag, int32_t* desc) {
  const bool neg = (value >> 63) != 0;
  if (kind == MRX_COL_FIXED) {
    uint64_t N;
    if (!format_fixed_scale(value, arg, &N)) return MRX_NUM_RANGE;
    const int nd = format_dec_digits(N);
    *mag = N;
    *desc = format_number_desc(neg, nd > arg + 1 ? nd : arg + 1, arg, false);
    return MRX_NUM_OK;
  }
  const bool hex = kind == MRX_COL_INT16;
  const uint64_t m = neg ? (uint64_t)0 - value : value;   // (INT64_MIN: 2^63, all its digits)
  const int nd = hex ? format_hex_digits(m) : format_dec_digits(m), K = arg > 1 ? arg : 1;
  *mag = m;
  *desc = format_number_desc(neg, nd > K ? nd : K, 0, hex);
  return MRX_NUM_OK;
}

// bytes [off, off + take) of a number cell (1 <= take <= 16, off + take <= its length) or-ed into a block at byte `at`
// (at + take <= 16).  The cell is up to four parts -- sign, digits in front of the point, point, digits behind it --
// and each part that the range meets is masked and shifted into place, as gather_place does with bytes from memory.
MRX_HD g_u128 format_place(g_u128 acc, uint64_t mag, int32_t desc, int off, int take, int at) {
  const int sign = (desc >> 5) & 1, digits = (desc >> 8) & 31, point = (desc >> 16) & 15;
  const FormatDigits d = format_digits(mag, ((desc >> 20) & 1) != 0);
  const int ip = digits - point;   // digits in front of the point
  if (sign) {
    if (off == 0) {
      acc |= (g_u128)'-' << (8 * at);
      ++at;
      --take;
    } else {
      --off;
    }
  }
  if (take > 0 && off < ip) {
    const int t = ip - off < take ? ip - off : take;
    g_u128 v = format_digits_window(d, 24 - digits + off);
    if (t < 16) v &= ((g_u128)1 << (8 * t)) - 1;
    acc |= v << (8 * at);
    at += t;
    take -= t;
    off = ip;
  }
  if (take > 0) {   // (off >= ip: only a cell with a point has bytes here)
    off -= ip;
    if (off == 0) {
      acc |= (g_u128)'.' << (8 * at);
      ++at;
      --take;
    } else {
      --off;
    }
    if (take > 0) {
      g_u128 v = format_digits_window(d, 24 - point + off);   // take <= point - off <= 9
      v &= ((g_u128)1 << (8 * take)) - 1;
      acc |= v << (8 * at);
    }
  }
  return acc;
}

// a whole number cell into out[0 .. its length): the per-cell formatter as one call (tests, tools)
MRX_HD int format_cell_bytes(uint64_t mag, int32_t desc, uint8_t* out) {
  const int len = format_desc_len(desc);
  for (int at = 0; at < len; at += 16) {
    const int take = len - at < 16 ? len - at : 16;
    const g_u128 v = format_place(0, mag, desc, at, take, 0);
    for (int q = 0; q < take; ++q) out[at + q] = (uint8_t)(v >> (8 * q));
  }
  return len;
}

// ---- the records --------------------------------------------------------------------------------------------------
// What the sizes kernel and the scan left for the gather.  The template's segments are expand's (ExpandSeg: a literal,
// or the slot of a referenced column); the cells of slot q lie at word[q * rows + r], desc[q * rows + r].
struct FormatSrc {
  const uint8_t* lits;      // the template's literals, 16-byte aligned, the words around them readable
  const ExpandSeg* segs;    // [nseg]
  int32_t nseg, pad_;
  int64_t rows;
  const uint64_t* word;     // [nslots][rows]
  const int32_t* desc;      // [nslots][rows]
  const int64_t* out_off;   // [rows + 1] CSR of the records
};

MRX_HD int64_t format_seg_len(const FormatSrc& S, const ExpandSeg& sg, int64_t r) {
  return sg.slot < 0 ? sg.lit_len : (int64_t)format_desc_len(S.desc[(int64_t)sg.slot * S.rows + r]);
}

// expand_block (mrx_expand_bits.hpp) with cells for groups: bytes [pos, endp) of the output, placed in the block that
// begins at output position p0 (p0 <= pos < endp <= p0 + 16).  r: the record that holds byte pos (never an empty one);
// hi: a record at or behind the one that holds byte endp - 1.
MRX_HD g_u128 format_block(const FormatSrc& S, int64_t r, int64_t hi, int64_t p0, int64_t pos, int64_t endp) {
  g_u128 acc = 0;
  while (true) {
    const int64_t s = S.out_off[r], e = S.out_off[r + 1];
    const int64_t lim = e < endp ? e : endp;
    int64_t off = pos - s;   // the segment walk: segments without a byte are passed
    int k = 0;
    for (; k + 1 < S.nseg; ++k) {
      const int64_t len = format_seg_len(S, S.segs[k], r);
      if (off < len) break;
      off -= len;
    }
    for (; pos < lim && k < S.nseg; ++k, off = 0) {
      const ExpandSeg sg = S.segs[k];
      int32_t desc = 0;
      uint64_t word = 0;
      int64_t left = sg.lit_len;
      if (sg.slot >= 0) {
        desc = S.desc[(int64_t)sg.slot * S.rows + r];
        left = format_desc_len(desc);
      }
      left -= off;
      if (left <= 0) continue;
      const int take = (int)(left < lim - pos ? left : lim - pos);
      if (sg.slot >= 0) word = S.word[(int64_t)sg.slot * S.rows + r];
      if (desc < 0) acc = format_place(acc, word, desc, (int)off, take, (int)(pos - p0));
      else acc = gather_place(acc, sg.slot < 0 ? S.lits + sg.lit_off + off : (const uint8_t*)(uintptr_t)word + off, take, (int)(pos - p0));
      pos += take;
    }
    pos = lim;   // (the segments of a record add up to its length: this changes nothing)
    if (pos >= endp) break;
    r = gather_gallop(S.out_off, r + 1, hi + 1, pos);
  }
  return acc;
}

}  // namespace mrx
