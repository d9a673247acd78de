// Event words -> spans: the expansion of one two-word event record of the streaming findall (k_decode's lean tile path).
// An event word F covers a 16-byte group: bit 2k = NEWSTART at byte k (a walk begins there), bit 2k + 1 = EMIT at byte k
// (a match ends in front of byte k: end = pb + k).  A record is {F of the even group, F of the odd group} of a pair that
// begins at text position pb, plus `rstart`, the start of the walk alive at the pair's first byte.  A match that ends at
// an EMIT began at the last NEWSTART strictly before that byte, or at rstart where the record has none there.
//
// The start without compare-and-select.  Claim: wherever a record has a NEWSTART in front of an EMIT,
// pb + (byte of that NEWSTART) >= rstart.  Proof: rstart is either 0 (no walk has begun yet) or the position of a NEWSTART
// the scan saw at an earlier byte of the same text than any byte of this pair (the scan sets it from the groups in front:
// `if (ns) start = gbase + last NEWSTART`), and a NEWSTART of this record lies at a text position >= 0 that is not before
// the pair's first event byte.  (The end-of-text record, whose rstart may lie INSIDE its pair, has no NEWSTART bit at
// all.)  Where the scan guarantees the two facts (k_stream_findall in mrx_kernels.hip; k_stream_dyn writes the same way):
//   * `start` is set to 0 when a lane takes a new text and changes only by `if (ns) start = gbase + ((31 - clz(ns)) >> 1)`
//     AFTER the group's record fields are taken (`sp_even = start | (gbase + kRecPosBias) << 16` / `rec12_pack(start, ..)`
//     at the even group), so a record's start is 0 or a NEWSTART of a group in front of the pair;
//   * bytes outside the text carry no event (`if (g * 16 + k >= lim || g * 16 + k < lo) e = q4;`), so every NEWSTART bit
//     lies at a text position >= 0;
//   * the end-of-text record ("end of text: a walk that is in an accepting state ends at len") is written as
//     `make_uint4(2u, 0u, start | (my_len + kRecPosBias) << 16, meta)` or, in 12 bytes, as the single bit
//     `2u << (2 * (my_len & 15))` in one word and 0 in the other: EMIT only.
// tests/test_gpu_decode_lean.py and the suite's parity tests compare the max form with the select form bit for bit on
// records the scan wrote.  So start = max(rstart, pb + index of the last NEWSTART before the EMIT) as long as "no NEWSTART" yields
// something <= rstart: clz_or_ones gives 0xFFFFFFFF for an empty mask -- one v_ffbh_u32 on the device, whose answer for 0
// is just that -- and pb + 15 - (0xFFFFFFFF >> 2) is below every position.  The same max carries the start from the
// even group into the odd one.
// Shared by k_decode and the host hook (mrx_testing_decode_expand), so the bit arithmetic is pinned without a GPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MRX_DECODE_HD __host__ __device__ inline
#else
#define MRX_DECODE_HD inline
#endif

namespace mrx {

constexpr uint32_t kEvEmitBits = 0xAAAAAAAAu, kEvNewstartBits = 0x55555555u;

// leading zeros of x, 0xFFFFFFFF for 0: one v_ffbh_u32 on the device, which answers just that.  The empty asm keeps the
// value whole: without it the compiler moves the caller's shift into both arms of the select and keeps a compare and a
// v_cndmask per span.
MRX_DECODE_HD uint32_t decode_clz_or_ones(uint32_t x) {
  uint32_t c = x ? (uint32_t)__builtin_clz(x) : ~0u;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(c));
#endif
  return c;
}
MRX_DECODE_HD int decode_max(int a, int b) { return a > b ? a : b; }

// pb15 + (index of the highest set bit, which sits at 2 j or 2 j + 1 for byte j) - 15, far below zero for an empty mask:
// bit 2 j -> clz 31 - 2 j -> 15 - j; bit 2 j + 1 -> clz 30 - 2 j -> 15 - j
// (an empty mask gives 0x3FFFFFFF to subtract: shift and mask are one v_bfe_u32, and the difference cannot wrap for any
// pb a record can hold -- 16 bits, from -143 where the pair's even group lies in front of a ragged text's frame)
MRX_DECODE_HD int decode_last_newstart(uint32_t mask, int pb15) {
  return pb15 - (int)((decode_clz_or_ones(mask) >> 1) & 0x3FFFFFFFu);
}

// the spans that end in one group, in text order: emit(start, end) for each.  rstart: the walk alive at the group's
// first byte.  FIXED: every match is fixed_len bytes long (an exact literal): start = end - fixed_len.
template <bool FIXED, class Emit>
MRX_DECODE_HD void decode_expand_group(uint32_t F, int pb, int rstart, int fixed_len, Emit& emit) {
  uint32_t em = F & kEvEmitBits;
  const uint32_t ns1 = (F & kEvNewstartBits) << 1;   // NEWSTART of byte j at bit 2 j + 1, where its EMIT is
  while (em) {
    const int b = __builtin_ctz(em);                 // 2 k + 1
    const int end = pb + (b >> 1);
    if (FIXED) emit(end - fixed_len, end);
    else emit(decode_max(rstart, decode_last_newstart(ns1 & ((1u << b) - 1u), pb + 15)), end);   // bytes j < k
    em &= em - 1;
  }
}

// one record (a pair of groups at text position pb) -> its spans in text order
template <bool FIXED, class Emit>
MRX_DECODE_HD void decode_expand_record(uint32_t f_even, uint32_t f_odd, int rstart, int pb, int fixed_len, Emit& emit) {
  decode_expand_group<FIXED>(f_even, pb, rstart, fixed_len, emit);
  if (!FIXED) rstart = decode_max(rstart, decode_last_newstart(f_even & kEvNewstartBits, pb + 15));
  decode_expand_group<FIXED>(f_odd, pb + 16, rstart, fixed_len, emit);
}

// ---- the tile's store loop, two spans per lane (k_decode<..., STORE16 = true>) ----
// A wavefront's spans are the absolute span indices pre0 .. pre0 + nspan - 1 of `spans`, 8 bytes each; the C ABI gives
// `spans` 8-byte alignment only.  Two consecutive spans leave as one 16-byte store where the first of them lies on a
// 16-byte boundary, that is where (address of spans / 8 + its index) is even.  odd = parity of that sum for the
// wavefront's first span; the kernel puts span k at tile slot k + odd, so that the pairs which are aligned in memory are
// aligned in the tile as well (one ds_read_b64 / ds_read_b128).  With odd the first span is the second half of a pair
// that belongs to the wavefront in front: it leaves alone (the head), and so does the last span where the count behind
// the head is odd (the tail).  Capacity is per span: only the nclip spans in front of span_cap leave, so a pair whose
// second span would sit at span_cap has become the tail.  Nothing at or behind span_cap and nothing in front of pre0 is
// part of the plan.  A later pass of a multi-pass wavefront calls this with pre0 + tb; TILE is even, so odd is the same
// in every pass.
struct DecodeStorePlan {
  int odd;      // span k of the wavefront sits at tile slot k + odd
  int nclip;    // spans that leave: min(nspan, span_cap - pre0), at least 0
  int head;     // 1: span 0 leaves with an 8-byte store (tile slot 1)
  int npairs;   // pair p = spans head + 2 p and head + 2 p + 1, tile slot odd + head + 2 p (even), one 16-byte store
  int tail;     // 1: span head + 2 npairs leaves with an 8-byte store
};
MRX_DECODE_HD int decode_store_odd(int64_t pre0, int addr_parity) { return (int)((pre0 + addr_parity) & 1); }
MRX_DECODE_HD DecodeStorePlan decode_store_plan(int64_t pre0, int addr_parity, int nspan, int64_t span_cap) {
  DecodeStorePlan pl;
  pl.odd = decode_store_odd(pre0, addr_parity);
  const int64_t room = span_cap - pre0;
  pl.nclip = room >= nspan ? nspan : room > 0 ? (int)room : 0;
  pl.head = pl.odd && pl.nclip > 0 ? 1 : 0;
  pl.npairs = (pl.nclip - pl.head) >> 1;
  pl.tail = (pl.nclip - pl.head) & 1;
  return pl;
}

}  // namespace mrx
