// Translate and strip (include/mrx.h, "translate", "strip"): bytes.translate plus tr -s, and bytes.strip as span rows.
// Host and device code: the walk of one aligned 16-byte block of a text is what k_translate_count and k_translate_emit
// run per lane (mrx_translate.hip), tr_map_block is what k_translate_map runs per lane and strip_text what k_strip runs,
// and mrx_debug_translate_host, mrx_debug_strip_host and tools/translate_check.cpp run the same functions on the CPU,
// block after block over the same pieces.
//
// Lookup: one table of 256 entries (mapped byte | flag bits), 16 lookups per block, in LDS on the device.  A second form
// that computed tables of at most 4 ranges [lo, hi] -> + delta with SWAR arithmetic on the 8-byte halves was built and
// measured against it: it won on no input (profiles/translate.md) and was taken out.
//
// Packed form (delete or squeeze).  A text is cut into pieces of P bytes as lines cuts it (mrx_lines_bits.hpp):
//   count   per piece: its kept bytes; one exclusive scan over the pieces
//   offsets pieces are text-major and texts leave in order, so out_offsets[i] is the scan at text i's first piece
//   emit    per piece: the kept, mapped bytes from the scan's entry of the piece on
// Squeeze looks one byte back: the mapped byte at q0 - 1, which is text whenever q0 > 0, so a run never reaches across
// a text boundary and a text's first byte is always kept.  (Delete and squeeze together would have to look back to the
// last surviving byte, any number of pieces away: refused.)
//
// Reading.  tr_block loads the aligned 16-byte words that hold a byte of its block inside the text and, under squeeze,
// the word of the byte in front of the block when that byte is text too.  Bytes of those words outside the text are
// masked before anything looks at them.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mrx.h"
#include "mrx_lines_bits.hpp"

namespace mrx {

constexpr int64_t kTranslatePiece = 4096;   // the piece without a pin (mrx_debug_translate_piece), as lines
enum { TR_MAP = 0, TR_DELETE = 1, TR_SQUEEZE = 2, TR_STRIP = 3 };
constexpr uint16_t kTrDelete = 0x100, kTrSqueeze = 0x200, kTrStrip = 0x400;   // flag bits of a table entry

struct TrPlan {
  uint32_t mode;
  uint16_t lut[256];   // entry c: table[c] | kTrDelete (c is deleted) | kTrSqueeze (table[c] is squeezed) | kTrStrip (c is
                       // stripped)
};

inline bool tr_bit(const uint8_t* bitmap, int c) { return bitmap && ((bitmap[c >> 3] >> (c & 7)) & 1); }
inline bool tr_any(const uint8_t* bitmap) {
  for (int k = 0; bitmap && k < 32; ++k)
    if (bitmap[k]) return true;
  return false;
}

// The plan of a call.  table: 256 bytes or NULL (the identity); del, sq, strip: 32-byte bitmaps or NULL, at most one of
// them with a member.
inline void tr_plan(const uint8_t* table, const uint8_t* del, const uint8_t* sq, const uint8_t* strip, TrPlan* P) {
  P->mode = tr_any(del) ? TR_DELETE : tr_any(sq) ? TR_SQUEEZE : tr_any(strip) ? TR_STRIP : TR_MAP;
  for (int c = 0; c < 256; ++c) {
    const int m = table ? table[c] : c;
    P->lut[c] = (uint16_t)(m | (tr_bit(del, c) ? kTrDelete : 0) | (tr_bit(sq, m) ? kTrSqueeze : 0) | (tr_bit(strip, c) ? kTrStrip : 0));
  }
}

// 16 bytes mapped through lut (the plan's table; in LDS on the device), and the 16-bit mask of the entries' flag `flag`
MRX_HD g_u128 tr_map16(const uint16_t* lut, g_u128 x, uint16_t flag, uint32_t* set) {
  uint64_t half[2] = {0, 0};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t e = lut[(uint32_t)(x >> (8 * k)) & 255u];
    half[k >> 3] |= (uint64_t)(e & 255u) << (8 * (k & 7));
    m |= (e & flag) ? 1u << k : 0u;
  }
  *set = m;
  return ((g_u128)half[1] << 64) | half[0];
}
MRX_HD g_u128 tr_low_bytes(g_u128 x, int v) { return v < 16 ? x & (((g_u128)1 << (8 * v)) - 1) : x; }

// one block: the mapped bytes and the 16-bit mask of those that go to the output
struct TrBlock {
  g_u128 bytes;
  uint32_t keep;
};
// The block at text position q0 (a multiple of 16, 0 <= q0 < L) of the text of L bytes at tp.
MRX_HD TrBlock tr_block(uint32_t mode, const uint16_t* lut, const uint8_t* tp, int64_t L, int64_t q0) {
  TrBlock b;
  const int v = L - q0 < 16 ? (int)(L - q0) : 16;
  const uint32_t valid = (1u << v) - 1u;
  const g_u128 x = tr_low_bytes(gather_window(tp + q0, v), v);
  uint32_t set = 0;
  b.bytes = tr_map16(lut, x, mode == TR_DELETE ? kTrDelete : mode == TR_SQUEEZE ? kTrSqueeze : (uint16_t)0, &set);
  b.keep = valid;
  if (mode == TR_DELETE) b.keep = valid & ~set;
  if (mode == TR_SQUEEZE) {
    uint32_t same = lines_eq16(b.bytes ^ (b.bytes << 8), 0) & ~1u;   // bit k: mapped byte k equals mapped byte k - 1
    if (q0 > 0 && (set & 1u)) {
      const uint32_t prev = lut[(uint32_t)gather_window(tp + q0 - 1, 1) & 255u] & 255u;
      same |= prev == ((uint32_t)b.bytes & 255u) ? 1u : 0u;
    }
    b.keep = valid & ~(set & same);
  }
  return b;
}

// ---- the same-length form: a lane per aligned 16-byte block of the output region -----------------------------------
// Block b of the region dst[0, N) (N > 0), counted from the last 16-byte boundary at or below dst: its bytes come from
// src at the same positions, through gather_window, so src and dst need not share an alignment.  A block inside the
// region goes out as one aligned 16-byte store, the first and the last one byte by byte: nothing outside the region
// is written, and only the aligned words that hold src[0, N) are read.
MRX_HD int64_t tr_map_blocks(const uint8_t* dst, int64_t N) { return (int64_t)(((uintptr_t)dst & 15) + (uintptr_t)N + 15) >> 4; }
MRX_HD void tr_map_block(const uint16_t* lut, const uint8_t* src, uint8_t* dst, int64_t N, int64_t b) {
  const uintptr_t a0 = (uintptr_t)dst & ~(uintptr_t)15;
  const int64_t head = (int64_t)((uintptr_t)dst - a0);
  const int64_t p0 = b * 16 - head, pos = p0 > 0 ? p0 : 0, endp = p0 + 16 < N ? p0 + 16 : N;
  const int v = (int)(endp - pos);
  uint32_t unused;
  const g_u128 y = tr_map16(lut, tr_low_bytes(gather_window(src + pos, v), v), 0, &unused);
  uint8_t* at = (uint8_t*)(a0 + (uintptr_t)b * 16);
  if (v == 16) {
    gather_store16(at, y);
  } else {
    for (int q = 0; q < v; ++q) at[(pos - p0) + q] = (uint8_t)(y >> (8 * q));
  }
}

// ---- strip: the aligned 16-byte words of a text from the front, then from the back ---------------------------------
// (start, end) of the text of L bytes at tp under the flags MRX_STRIP_LEFT | MRX_STRIP_RIGHT.  Only the words that hold
// a stripped byte or the first byte that stays are loaded at either end: a text of set bytes alone is walked whole.
MRX_HD void strip_text(const uint16_t* lut, const uint8_t* tp, int64_t L, uint32_t flags, int64_t* start, int64_t* end) {
  *start = 0, *end = L;
  if (L <= 0) { *end = 0; return; }
  const int head = (int)((uintptr_t)tp & 15);
  const uint8_t* base = tp - head;
  const int64_t nwords = (head + L + 15) >> 4;
  // the set's mask over word wi, its bytes outside the text taken out first
  auto others = [&](int64_t wi) {
    const int64_t lo = 16 * wi - head;   // text position of the word's first byte
    const int from = lo < 0 ? (int)-lo : 0, to = L - lo < 16 ? (int)(L - lo) : 16;
    const uint32_t valid = ((1u << to) - 1u) & ~((1u << from) - 1u);
    g_u128 x = gather_window(base + 16 * wi, 16);
    x = tr_low_bytes(x, to) >> (8 * from) << (8 * from);
    uint32_t set = 0;
    (void)tr_map16(lut, x, kTrStrip, &set);
    return valid & ~set;   // the text's bytes that stay
  };
  if (flags & MRX_STRIP_LEFT) {
    *start = L;
    for (int64_t wi = 0; wi < nwords; ++wi) {
      const uint32_t m = others(wi);
      if (m) {
#if defined(__HIP_DEVICE_COMPILE__)
        *start = 16 * wi - head + (__ffs((int)m) - 1);
#else
        *start = 16 * wi - head + __builtin_ctz(m);
#endif
        break;
      }
    }
  }
  if ((flags & MRX_STRIP_RIGHT) && *start < L) {
    *end = *start;   // (with MRX_STRIP_LEFT the byte at start stays: the walk ends there at the latest)
    for (int64_t wi = nwords - 1; wi >= 0 && 16 * wi - head + 16 > *start; --wi) {
      uint32_t m = others(wi);
      const int64_t lo = 16 * wi - head;
      if (*start > lo) m &= ~((1u << (int)(*start - lo)) - 1u);
      if (m) {
#if defined(__HIP_DEVICE_COMPILE__)
        *end = lo + (32 - __clz((int)m));
#else
        *end = lo + (32 - __builtin_clz(m));
#endif
        break;
      }
    }
  }
}

// ---- host only: the passes, piece by piece as the kernels take them --------------------------------------------------
struct TrHostOut {
  int64_t* out_offsets;   // [n + 1]
  uint8_t* out_data;
  int64_t out_cap;
  int64_t* totals;        // [2]
};

// Text i is data[off[i], off[i + 1]); the aligned 16-byte words around every text must be readable.  Writes what the
// contract of mrx_translate_dev says the packed form writes, under its capacity rule, and nothing else.
inline void translate_host(const TrPlan& Pl, const uint8_t* data, const int64_t* off, int64_t n, int64_t P, const TrHostOut& o) {
  const TextBatch B = csr(data, off);
  std::vector<int64_t> first((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    int64_t L;
    (void)lines_text(B, i, &L);
    first[(size_t)i + 1] = first[(size_t)i] + lines_pieces_of(L, P);
  }
  const int64_t np = first[(size_t)n];
  std::vector<int64_t> scan((size_t)np + 1, 0);
  for (int64_t i = 0; i < n; ++i) {   // count
    int64_t L;
    const uint8_t* tp = lines_text(B, i, &L);
    for (int64_t p = first[(size_t)i]; p < first[(size_t)i + 1]; ++p) {
      const int64_t p0 = (p - first[(size_t)i]) * P, pend = p0 + P < L ? p0 + P : L;
      int64_t kept = 0;
      for (int64_t q0 = p0; q0 < pend; q0 += 16) kept += lines_popc(tr_block(Pl.mode, Pl.lut, tp, L, q0).keep);
      scan[(size_t)p + 1] = scan[(size_t)p] + kept;
    }
  }
  int64_t longest = 0;
  for (int64_t i = 0; i <= n; ++i) {   // offsets
    o.out_offsets[i] = scan[(size_t)first[(size_t)i]];
    if (i > 0 && o.out_offsets[i] - o.out_offsets[i - 1] > longest) longest = o.out_offsets[i] - o.out_offsets[i - 1];
  }
  o.totals[0] = scan[(size_t)np];
  o.totals[1] = longest;
  if (o.totals[0] > o.out_cap) return;
  for (int64_t i = 0; i < n; ++i) {   // emit
    int64_t L;
    const uint8_t* tp = lines_text(B, i, &L);
    for (int64_t p = first[(size_t)i]; p < first[(size_t)i + 1]; ++p) {
      const int64_t p0 = (p - first[(size_t)i]) * P, pend = p0 + P < L ? p0 + P : L;
      int64_t pos = scan[(size_t)p];
      for (int64_t q0 = p0; q0 < pend; q0 += 16) {
        const TrBlock b = tr_block(Pl.mode, Pl.lut, tp, L, q0);
        for (int k = 0; k < 16; ++k)
          if ((b.keep >> k) & 1u) o.out_data[pos++] = (uint8_t)(b.bytes >> (8 * k));
      }
    }
  }
}
// the same-length form over the region dst[0, N) from src[0, N), block after block
inline void translate_map_host(const TrPlan& Pl, const uint8_t* src, uint8_t* dst, int64_t N) {
  if (N <= 0) return;
  const int64_t nblk = tr_map_blocks(dst, N);
  for (int64_t b = 0; b < nblk; ++b) tr_map_block(Pl.lut, src, dst, N, b);
}
// rows[i] = (start, end) of text i
inline void strip_host(const TrPlan& Pl, const uint8_t* data, const int64_t* off, int64_t n, uint32_t flags, int32_t* rows) {
  const TextBatch B = csr(data, off);
  for (int64_t i = 0; i < n; ++i) {
    int64_t L, s, e;
    const uint8_t* tp = lines_text(B, i, &L);
    strip_text(Pl.lut, tp, L, flags, &s, &e);
    rows[2 * i] = (int32_t)s, rows[2 * i + 1] = (int32_t)e;
  }
}

}  // namespace mrx
