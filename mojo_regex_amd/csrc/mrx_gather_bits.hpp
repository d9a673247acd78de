// What the output-centric byte movers share (mrx_filter.hip, mrx_extract.hip, mrx_expand.hip, mrx_format.hip): a lane owns
// one 16-byte block of the output, aligned on the output ADDRESS, finds the row that holds the block's first byte in the
// output's CSR and fills the block from that row's source and the following ones.  The block assembly (window, place,
// store, the two searches) is host and device code: it also runs on the CPU against memcpy (tools/extract_block_check.cpp,
// expand_block_check.cpp, format_check.cpp, each with a sequential loop over the blocks of its own).  The walk that gives
// every lane its block, gather_blocks at the end of this file, is device code and the only copy of it.
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

#if defined(__HIPCC__)
// The block walk of a gather kernel launched with workgroups of kBlock lanes: out[0, bytes) (bytes > 0) is cut into
// 16-byte blocks aligned on out's address, and off[rows + 1] is its CSR (off[rows] = bytes).  A wavefront takes one
// contiguous run of blocks, 64 per round: it bisects all rows once for its first block, then per round gallops forward
// from the last round's row to the row of the round's last byte (uniform, broadcast loads), and each lane bisects only
// the rows between the two.  fill(r, hi, p0, pos, endp) returns the lane's block: bytes [pos, endp) of the output, byte
// p of it at block position p - p0 (p0 <= pos < endp <= p0 + 16); row r holds byte pos and row hi the round's last
// byte (off[rows] = bytes > pos: r stays below rows).  A block inside the output goes out as one aligned 16-byte store;
// only the first block (an unaligned out) and the last one (the end of the output) are written byte by byte, so nothing
// outside [0, bytes) is touched.
template <int kBlock, class Fill>
__device__ __forceinline__ void gather_blocks(uint8_t* out, int64_t bytes, const int64_t* off, int64_t rows, const Fill& fill) {
  const uintptr_t ob = (uintptr_t)out, a0 = ob & ~(uintptr_t)15;
  const int64_t head = (int64_t)(ob - a0);   // output position p lies in block (p + head) / 16
  const int64_t nblk = (head + bytes + 15) >> 4;
  const int lane = (int)threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64), w = (int64_t)blockIdx.x * (kBlock / 64) + ((int)threadIdx.x >> 6);
  const int64_t per = ((nblk + nw - 1) / nw + 63) & ~(int64_t)63;
  const int64_t b_begin = w * per, b_end = b_begin + per < nblk ? b_begin + per : nblk;
  if (b_begin >= b_end) return;
  const int64_t p_first = b_begin * 16 - head;
  int64_t cur = gather_last_le(off, 0, rows, p_first > 0 ? p_first : 0);
  for (int64_t b0 = b_begin; b0 < b_end; b0 += 64) {
    const int64_t bl = b0 + 63 < b_end ? b0 + 63 : b_end - 1;
    const int64_t pe = bl * 16 - head + 15, pl = pe < bytes ? pe : bytes - 1;   // the round's last byte
    const int64_t hi = gather_gallop(off, cur, rows, pl);
    const int64_t b = b0 + lane;
    if (b <= bl) {
      const int64_t p0 = b * 16 - head;
      const int64_t pos = p0 > 0 ? p0 : 0;
      const int64_t endp = p0 + 16 < bytes ? p0 + 16 : bytes;
      const g_u128 acc = fill(gather_last_le(off, cur, hi + 1, pos), hi, p0, pos, endp);
      uint8_t* dst = (uint8_t*)(a0 + (uintptr_t)b * 16);
      if (p0 >= 0 && p0 + 16 <= bytes) {
        gather_store16(dst, acc);
      } else {   // the first block of an unaligned output, the last block of the output
        for (int q = p0 < 0 ? (int)-p0 : 0; q < (int)(endp - p0); ++q) dst[q] = (uint8_t)(acc >> (8 * q));
      }
    }
    cur = hi;
  }
}
#endif

}  // namespace mrx
