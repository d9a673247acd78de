// What the output-centric byte movers share (mrx_filter.hip, mrx_extract.hip, mrx_expand.hip): a lane owns one 16-byte block of
// the output, aligned on the output ADDRESS, finds the piece that holds the block's first byte in the output's CSR and
// fills the block from that piece's source and the following ones.  Host and device: the block assembly also runs on
// the CPU against memcpy (tools/extract_block_check.cpp).
#pragma once
#include <cstdint>

#include "mrx_internal.hpp"

namespace mrx {

typedef unsigned __int128 g_u128;
typedef uint64_t g_u64x2 __attribute__((ext_vector_type(2)));

// bytes p[0 .. 16) as one little-endian value; only the first `need` (1 .. 16) are meaningful, and only the aligned
// 16-byte words that hold one of them are loaded (p[0 .. need) lies inside a text)
MRX_HD g_u128 gather_window(const uint8_t* p, int need) {
  const uintptr_t a = (uintptr_t)p;
  const g_u64x2* w = (const g_u64x2*)(a & ~(uintptr_t)15);
  const int sh = (int)(a & 15);
  const g_u64x2 x = w[0];
  const g_u128 lo = ((g_u128)x.y << 64) | x.x;
  if (sh == 0) return lo;
  g_u128 hi = 0;
  if (sh + need > 16) {
    const g_u64x2 y = w[1];
    hi = ((g_u128)y.y << 64) | y.x;
  }
  return (lo >> (8 * sh)) | (hi << (128 - 8 * sh));
}
MRX_HD void gather_store16(uint8_t* aligned, g_u128 v) {
  g_u64x2 x;
  x.x = (uint64_t)v;
  x.y = (uint64_t)(v >> 64);
  *(g_u64x2*)aligned = x;
}
// a block with src[0 .. take) or-ed in at its byte `at` (1 <= take, at + take <= 16): window, mask, shift
MRX_HD g_u128 gather_place(g_u128 acc, const uint8_t* src, int take, int at) {
  g_u128 v = gather_window(src, take);
  if (take < 16) v &= ((g_u128)1 << (8 * take)) - 1;
  return acc | (v << (8 * at));
}

// the last r in [a, b) with off[r] <= p (off[a] <= p)
MRX_HD int64_t gather_last_le(const int64_t* __restrict__ off, int64_t a, int64_t b, int64_t p) {
  while (b - a > 1) {
    const int64_t mid = (a + b) >> 1;
    if (off[mid] <= p) a = mid; else b = mid;
  }
  return a;
}

// the last q in [a, b) with off[q] <= p (off[a] <= p), by doubling steps from a: cheap when q is close to a
MRX_HD int64_t gather_gallop(const int64_t* __restrict__ off, int64_t a, int64_t b, int64_t p) {
  int64_t step = 1;
  while (a + step < b && off[a + step] <= p) {
    a += step;
    step <<= 1;
  }
  return gather_last_le(off, a, a + step < b ? a + step : b, p);
}

}  // namespace mrx
