// Expand's record assembly (mrx_expand.hip): a record is a template's segments back to back -- a literal from the
// literal buffer, or a group of the record's row from its text -- and a lane of the gather owns one 16-byte block of
// the packed records.  The segment walk (record position -> segment, offset in it) and the block assembly are host and
// device code, so that they also run on the CPU against a byte-by-byte build (tools/expand_block_check.cpp).
#pragma once
#include <cstdint>

#include "mrx_gather_bits.hpp"

namespace mrx {

// one segment of a parsed template, as the kernels read it
struct ExpandSeg {
  int64_t lit_off;   // a literal: its first byte in the literal buffer ...
  int64_t lit_len;   // ... and its length (> 0)
  int32_t slot;      // a group: the slot of its clamped pair in the row's source entry; -1: a literal
  int32_t pad_;
};

// what the sizes kernel and the scan left for the gather
struct ExpandSrc {
  const uint8_t* data;      // the batch's bytes
  const uint8_t* lits;      // the template's literals, 16-byte aligned, the words around them readable
  const ExpandSeg* segs;    // [nseg]
  int32_t nseg, nslots;
  const int64_t* base;      // [rows] absolute position in `data` of the row's text
  const int32_t* pairs;     // [rows][nslots][2] the referenced groups of each row, clamped to its text: (s', e')
  const int64_t* out_off;   // [rows + 1] CSR of the records
};

MRX_HD int64_t expand_seg_len(const ExpandSeg& sg, const int32_t* pairs) {
  return sg.slot < 0 ? sg.lit_len : (int64_t)(pairs[2 * sg.slot + 1] - pairs[2 * sg.slot]);
}

// The segment walk: byte q of a record (0 <= q < its length) lies in segment *k, at the returned offset.  Segments
// without a byte (an unset group) are passed.  The record's length is the sum of its segments' lengths, so the walk
// ends inside the table; it never steps past the last entry.
MRX_HD int64_t expand_seek(const ExpandSeg* segs, int nseg, const int32_t* pairs, int64_t q, int* k) {
  int i = 0;
  for (; i + 1 < nseg; ++i) {
    const int64_t len = expand_seg_len(segs[i], pairs);
    if (q < len) break;
    q -= len;
  }
  *k = i;
  return q;
}

// Bytes [pos, endp) of the output, placed in the block that begins at output position p0 (p0 <= pos < endp <= p0 + 16).
// r: the record that holds byte pos (never an empty one); hi: a record at or behind the one that holds byte endp - 1.
// Inside a record the segments are taken one after the other with gather_place; at a record's end the next record with
// a byte is found by galloping (an empty record repeats its offset).
MRX_HD g_u128 expand_block(const ExpandSrc& S, int64_t r, int64_t hi, int64_t p0, int64_t pos, int64_t endp) {
  g_u128 acc = 0;
  while (true) {
    const int64_t s = S.out_off[r], e = S.out_off[r + 1];
    const int64_t lim = e < endp ? e : endp;
    const int32_t* pr = S.pairs + 2 * r * S.nslots;
    int k;
    int64_t off = expand_seek(S.segs, S.nseg, pr, pos - s, &k);
    for (; pos < lim && k < S.nseg; ++k, off = 0) {
      const ExpandSeg sg = S.segs[k];
      const int64_t left = expand_seg_len(sg, pr) - off;
      if (left <= 0) continue;
      const int take = (int)(left < lim - pos ? left : lim - pos);
      const uint8_t* src = sg.slot < 0 ? S.lits + sg.lit_off + off : S.data + S.base[r] + pr[2 * sg.slot] + off;
      acc = gather_place(acc, src, take, (int)(pos - p0));
      pos += take;
    }
    pos = lim;   // (the segments of a record add up to its length: this changes nothing)
    if (pos >= endp) break;
    r = gather_gallop(S.out_off, r + 1, hi + 1, pos);
  }
  return acc;
}

}  // namespace mrx
