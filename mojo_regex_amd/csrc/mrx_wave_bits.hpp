// Cross-lane sums on the DPP path, for the kernels of more than one unit (the findall decode, sub): device code only,
// inlined where it is used.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mrx {
// Inclusive scan over the G lanes of a group (16, 32 or 64: groups are aligned rows of 16 lanes) on the
// DPP path: row_shr 1 / 2 / 4 / 8 inside a row, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2
// and 3 -- one VALU instruction per step where __shfl_up costs a ds_bpermute round trip and a select.
template <int G, bool XOR>
__device__ __forceinline__ int group_scan(int x) {
#define MRX_DPP_STEP(CTRL, ROWS)                                                      \
  do {                                                                                \
    const int y = __builtin_amdgcn_update_dpp(0, x, CTRL, ROWS, 0xF, false);          \
    x = XOR ? (x ^ y) : (x + y);                                                      \
  } while (0)
  MRX_DPP_STEP(0x111, 0xF);   // row_shr:1
  MRX_DPP_STEP(0x112, 0xF);   // row_shr:2
  MRX_DPP_STEP(0x114, 0xF);   // row_shr:4
  MRX_DPP_STEP(0x118, 0xF);   // row_shr:8
  if (G >= 32) MRX_DPP_STEP(0x142, 0xA);   // row_bcast:15 -> rows 1, 3
  if (G >= 64) MRX_DPP_STEP(0x143, 0xC);   // row_bcast:31 -> rows 2, 3
#undef MRX_DPP_STEP
  return x;
}

// Sum over the wavefront of one 64-bit value per lane -- none negative, the total below 2^63 -- as a wave-uniform
// value: three 32-bit DPP scans (the low word as two 16-bit halves, which 64 lanes cannot overflow, and the high
// word) whose last lane is read into SGPRs.  No LDS round trip.
__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)((uint64_t)v >> 32);
  const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane(group_scan<64, false>((int)(lo & 0xFFFFu)), 63);
  const uint32_t s1 = (uint32_t)__builtin_amdgcn_readlane(group_scan<64, false>((int)(lo >> 16)), 63);
  const uint32_t s2 = (uint32_t)__builtin_amdgcn_readlane(group_scan<64, false>((int)hi), 63);
  return (int64_t)((uint64_t)s0 + ((uint64_t)s1 << 16) + ((uint64_t)s2 << 32));
}
}  // namespace mrx
