// The groups of a deterministic chain (HostPlan::chain) on the device, for the kernels that read them: sub() with
// \1..\9 (k_subc_sizes / k_subc_emit, mrx_sub.hip) and captures_all (k_capall_chain, mrx_capall.hip).  A wavefront
// takes a text: every byte's leaf mask in an LDS tile (subc_store), a lane per match finds the leaves' boundaries as
// runs of mask bits (subc_walk).  Device code only, inlined where it is used.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mrx_plan.hpp"

namespace mrx {
constexpr int kSubcLeaves = 8, kSubcTpl = 8, kSubcRepl = 256;   // (loops over leaves and segments are unrolled: the kernel
                                                                   // arguments they index stay in scalar registers)
struct ChainDev {
  int nleaf, ntpl;
  int lmax[kSubcLeaves];
  int lfix[kSubcLeaves];   // width of a leaf with a fixed count, else 0
  int need;                // bit l: leaf l's runs are looked at (variable count, not the last leaf): its bitmap is built
  ReplSeg tpl[kSubcTpl];   // (as sub_chain_from_spans rewrites them: a group's segment names its two boundaries)
};
// One text's descriptor, loaded two texts ahead; its blocks, first spans and first gains one text ahead: the global
// round trips of text i + 1 run under the LDS phases of text i (as in k_subs_wave).
struct SubcDesc { int64_t ibase, a, obase; int tlen, k, olen; };
template <bool EMIT>
__device__ __forceinline__ SubcDesc subc_desc(int64_t i, int64_t n, const int64_t* offsets, const int64_t* prefix,
                                              const int64_t* out_off, long long count) {
  SubcDesc d{0, 0, 0, 0, 0, 0};
  if (i < n) {
    d.ibase = offsets[i];
    d.tlen = (int)(offsets[i + 1] - d.ibase);
    d.a = prefix[i];
    int64_t k64 = prefix[i + 1] - d.a;
    if (count > 0 && k64 > count) k64 = count;
    d.k = (int)k64;
    if constexpr (EMIT) {
      d.obase = out_off[i];
      d.olen = (int)(out_off[i + 1] - d.obase);
    }
  }
  return d;
}
// blocks in registers -> per-leaf bitmaps (bm[l * ROW + b] bit j: leaf l takes byte 16 b + j of the frame) and, when wanted,
// the text tile; frame of the blocks: the text begins at [address & 15]
template <int NB, int ROW, bool TEXT>
__device__ __forceinline__ void subc_store(const uint4 (&tx)[NB], uint16_t* bm, uint8_t* tile, const uint8_t* mask, int need,
                                           int nfb, int lane) {
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    const int b = lane + 64 * r;
    if (b < nfb) {
      const uint4 v = tx[r];
      if constexpr (TEXT) *(uint4*)(tile + 16 * b) = v;
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      uint32_t o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        o[q] = (uint32_t)mask[w[q] & 255] | ((uint32_t)mask[(w[q] >> 8) & 255] << 8) |
               ((uint32_t)mask[(w[q] >> 16) & 255] << 16) | ((uint32_t)mask[w[q] >> 24] << 24);
#pragma unroll
      for (int l = 0; l < kSubcLeaves; ++l) {
        if (!((need >> l) & 1)) continue;
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)   // bit l of four bytes -> four adjacent bits (the products' other terms stay below bit 24)
          bits |= (((((o[q] >> l) & 0x01010101u) * 0x01020408u) >> 24) & 15u) << (4 * q);
        bm[l * ROW + b] = (uint16_t)bits;
      }
    }
  }
}
// boundaries of the leaves of the match [ms, me) -> bnd[0 .. nleaf] (the lane's row); positions relative to the text, which
// begins at frame position mis; a leaf's run: trailing ones of its bitmap from the position on, 32 positions a step
template <int ROW>
__device__ __forceinline__ void subc_walk(const ChainDev& cd, const uint16_t* bm, int mis, uint16_t* bnd, int ms, int me) {
  int pos = ms;
#pragma unroll
  for (int l = 0; l < kSubcLeaves; ++l) {
    if (l >= cd.nleaf) break;
    bnd[l] = (uint16_t)pos;
    if (l == cd.nleaf - 1) { pos = me; break; }          // the last leaf ends with the match
    if (cd.lfix[l]) { pos += cd.lfix[l]; continue; }     // a fixed count: nothing to look at (the match is the table walk's)
    const int lm = cd.lmax[l];
    const int stop = lm < 0 || pos + lm > me ? me : pos + lm;
    const uint16_t* row = bm + l * ROW;
    while (pos < stop) {
      const int f = mis + pos;
      const uint16_t* w = row + (f >> 4);
      const uint32_t lo = (uint32_t)w[0] | ((uint32_t)w[1] << 16), hi = w[2];
      const uint32_t miss = ~__funnelshift_r(lo, hi, f & 15);
      int k = miss ? __ffs((int)miss) - 1 : 32;
      if (k > stop - pos) k = stop - pos;
      pos += k;
      if (k < 32) break;
    }
  }
  bnd[cd.nleaf] = (uint16_t)pos;
}
// (ChainDev::tpl as the host rewrote it: group_ref != 0: bytes between the boundaries `start` and `length`; else literal)
__device__ __forceinline__ int subc_repl_len(const ChainDev& cd, const uint16_t* bnd) {
  int rl = 0;
#pragma unroll
  for (int k = 0; k < kSubcTpl; ++k) {
    if (k >= cd.ntpl) break;
    const ReplSeg sg = cd.tpl[k];
    rl += sg.group_ref ? (int)bnd[sg.length] - (int)bnd[sg.start] : sg.length;
  }
  return rl;
}
// n bytes src -> dst (LDS, one lane), four reads in flight
__device__ __forceinline__ void subc_copy(uint8_t* dst, const uint8_t* src, int n) {
  for (int j = 0; j < n; j += 4) {
    const uint8_t b0 = src[j], b1 = src[j + 1], b2 = src[j + 2], b3 = src[j + 3];   // (the tiles are padded)
    dst[j] = b0;
    if (j + 1 < n) dst[j + 1] = b1;
    if (j + 2 < n) dst[j + 2] = b2;
    if (j + 3 < n) dst[j + 3] = b3;
  }
}
#define MRX_SUBC_WAVE_SYNC()                                      \
  do {                                                            \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        \
    __builtin_amdgcn_wave_barrier();                              \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");        \
  } while (0)
}  // namespace mrx
