// What the piece-wise packers share (mrx_lines.hip, mrx_translate.hip): the cut of a batch's texts into text-major pieces
// of P bytes, the wavefront's way from a piece to its text, and the LDS stage through which a wavefront's kept bytes
// leave as aligned 16-byte blocks.  Device code and the launches around it; the block walks themselves are in
// mrx_lines_bits.hpp and mrx_translate_bits.hpp.
//
// Pieces are numbered text-major.  Fixed pitch: every text has ceil(longest / P) of them (1 at least), so piece -> text is
// a division.  CSR: a search of the texts' first pieces by the whole wavefront; the grid is sized by an upper bound of
// the piece count (bytes / P + n, the bytes from the caller's known bound or from one read-back of the first and last
// offset), and the pieces beyond the last text's hold nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_lines_bits.hpp"

namespace mrx {

// the pieces of a call
struct LinesPieces {
  int64_t P;
  int64_t per_text;       // fixed pitch: pieces of every text
  const int64_t* first;   // CSR: [n + 1], the first piece of every text
  int64_t npieces;        // to walk (CSR: an upper bound)
};
// bytes [p0, pend) of text `text` (pend == p0: nothing); a: the text's first piece
struct LinesJob {
  const uint8_t* tp;
  int64_t L, p0, pend, text, a;
};

// gather_last_le(first, 0, n, piece) by a whole wavefront (every lane calls it with the same arguments): each round the
// lanes probe 64 evenly spaced entries of what is left, so a million texts take four dependent loads, not twenty.  The
// lanes whose entry is at or below `piece` are a prefix of the wavefront (first[] does not decrease, first[lo] <= piece).
__device__ __forceinline__ int64_t lines_wave_last_le(const int64_t* __restrict__ first, int64_t n, int64_t piece) {
  const int lane = (int)threadIdx.x & 63;
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t step = (hi - lo + 63) >> 6, idx = lo + lane * step;
    const unsigned long long at_or_below = __ballot(idx < hi && first[idx] <= piece);
    const int64_t k = __popcll(at_or_below | 1ull) - 1;
    lo += k * step;
    hi = lo + step < hi ? lo + step : hi;
  }
  return lo;
}

__device__ __forceinline__ LinesJob lines_job(const TextBatch& B, int64_t n, const LinesPieces& pc, int64_t piece) {
  LinesJob j{nullptr, 0, 0, 0, 0, 0};
  if (piece >= pc.npieces) return j;
  if (pc.first) {
    if (piece >= pc.first[n]) return j;
    j.text = lines_wave_last_le(pc.first, n, piece);   // (empty texts repeat the value: the last one has the piece)
    j.a = pc.first[j.text];
  } else {
    j.text = piece / pc.per_text;
    j.a = j.text * pc.per_text;
  }
  j.tp = lines_text(B, j.text, &j.L);
  j.p0 = j.pend = (piece - j.a) * pc.P;
  if (j.p0 < j.L) j.pend = j.p0 + pc.P < j.L ? j.p0 + pc.P : j.L;
  return j;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int off = 32; off > 0; off >>= 1) {
    const int y = __shfl_xor(v, off);
    v = y > v ? y : v;
  }
  return v;
}

static __global__ __launch_bounds__(256) void k_lines_pieces(const TextBatch B, int64_t n, int64_t P, int64_t* __restrict__ per) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t L;
    (void)lines_text(B, i, &L);
    per[i] = lines_pieces_of(L, P);
  }
}

// The pieces of a checked batch of n >= 1 texts: pc->P is set, the rest is filled in.  known_total: a CSR batch's byte
// count where the caller has it (an upper bound is fine), < 0: the first and last offset are read back, which `syncs`
// counts.  dummy: a device word for the sum of the scan that nobody reads.  Scratch comes from the caller's scope.
inline int lines_pieces_setup(const TextBatch& b, int64_t n, int64_t known_total, int64_t* dummy, std::atomic<int64_t>& syncs,
                              void* stream, LinesPieces* pc) {
  hipStream_t hs = (hipStream_t)stream;
  if (b.offsets) {
    int64_t bytes = known_total;
    if (bytes < 0) {
      int64_t ends[2] = {0, 0};
      MRX_HIP_TRY(hipMemcpyAsync(&ends[0], b.offsets, sizeof(int64_t), hipMemcpyDeviceToHost, hs));
      MRX_HIP_TRY(hipMemcpyAsync(&ends[1], b.offsets + n, sizeof(int64_t), hipMemcpyDeviceToHost, hs));
      MRX_HIP_TRY(hipStreamSynchronize(hs));   // the piece count sizes the scratch
      ++syncs;
      if (ends[1] < ends[0]) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
      bytes = ends[1] - ends[0];
    }
    int64_t* per = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, stream);
    int64_t* first = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), stream);
    if (!per || !first) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
    hipLaunchKernelGGL(k_lines_pieces, dim3(grid_for(n, 256, 4096)), dim3(256), 0, hs, b, n, pc->P, per);
    MRX_HIP_TRY(hipGetLastError());
    if (int rc = exclusive_scan(per, n, first, dummy, stream)) return rc;
    pc->first = first;
    pc->npieces = bytes / pc->P + n;   // ceil(len / P) <= len / P + 1 for every text
  } else {
    pc->per_text = lines_pieces_of(b.pitch_longest(), pc->P);
    if (pc->per_text < 1) pc->per_text = 1;
    pc->npieces = n * pc->per_text;
  }
  return MRX_OK;
}

// ---- the stage ------------------------------------------------------------------------------------------------------
// An emit kernel moves no output byte to memory on its own.  A lane drops its kept bytes into its wavefront's LDS stage
// at the place the wave's prefix sum gives them -- the stage is laid out like the output from the last 16-byte boundary
// of its ADDRESS on -- and the lanes then store the stage's complete 16-byte blocks, aligned, one a lane.  What is left
// behind the last complete block stays in the stage for the next round.  Only the two ends of a piece, blocks that it
// shares with the pieces around it, go out as single bytes, a lane each: no block has two writers of one byte.
constexpr int kLinesStage = (int)kLinesRound + 32;   // a round's bytes behind at most 15 held over, in whole blocks

// A stage belongs to one wavefront, whose LDS accesses the hardware serves in program order: what the lanes need between
// writing the stage and reading it is that the compiler keeps that order, not a barrier of the workgroup.
__device__ __forceinline__ void lines_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the stage holds the output from the address `ablk` (16-byte aligned) on: [own, fill) are bytes of this piece that no
// block has taken yet, [0, own) belong to the piece in front
struct LinesStage {
  uintptr_t ablk;
  int fill, own;
};
// a piece whose first kept byte goes to out[pos] (on == false: a piece that moves nothing)
__device__ __forceinline__ LinesStage lines_stage_open(bool on, uint8_t* out, int64_t pos) {
  LinesStage s{0, 0, 0};
  if (on) {
    const uintptr_t addr = (uintptr_t)out + (uintptr_t)pos;
    s.ablk = addr & ~(uintptr_t)15;
    s.fill = s.own = (int)(addr & 15);
  }
  return s;
}
// One round of an open stage, all 64 lanes: the lane's kept bytes (`keep` over `bytes`) go behind the kept_before bytes
// of the lanes below, K bytes in the round; the complete blocks leave.
__device__ __forceinline__ void lines_stage_round(LinesStage& s, g_u64x2* stage16, int lane, g_u128 bytes, uint32_t keep,
                                                  int kept_before, int K) {
  uint8_t* stage = (uint8_t*)stage16;
  uint8_t* w = stage + s.fill + kept_before;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if ((keep >> k) & 1u) *w++ = (uint8_t)(bytes >> (8 * k));
  lines_wave_sync();
  const int have = s.fill + K, nb = have >> 4, rem = have & 15;
  if (lane < nb) {
    if (lane > 0 || s.own == 0) gather_store16((uint8_t*)(s.ablk + 16 * (uintptr_t)lane), ((g_u128)stage16[lane].y << 64) | stage16[lane].x);
  }
  if (nb > 0 && lane >= s.own && lane < 16 && s.own > 0) *(uint8_t*)(s.ablk + (uintptr_t)lane) = stage[lane];
  const uint8_t held = lane < rem ? stage[16 * nb + lane] : (uint8_t)0;
  lines_wave_sync();
  if (nb > 0) {
    if (lane < rem) stage[lane] = held;
    s.ablk += 16 * (uintptr_t)nb;
    s.own = 0;
  }
  s.fill = rem;
}
// behind a piece's last round: what is left is the piece's share of a block that the next piece goes on with
__device__ __forceinline__ void lines_stage_close(const LinesStage& s, g_u64x2* stage16, int lane) {
  const uint8_t* stage = (const uint8_t*)stage16;
  lines_wave_sync();
  if (lane >= s.own && lane < s.fill) *(uint8_t*)(s.ablk + (uintptr_t)lane) = stage[lane];
  lines_wave_sync();
}

}  // namespace mrx
