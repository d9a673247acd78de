// Translate and strip (include/mrx.h, "translate", "strip"): bytes.translate plus tr -s for every text of a batch as a
// new batch on the device, and bytes.strip as span rows.  The block walks, the lookup and the order of the
// passes are in mrx_translate_bits.hpp; here are the kernels, the launches and the entry points.
//
//   k_translate_map       same-length form: a lane per aligned 16-byte block of the output region; one launch, no scratch
//   k_translate_count     packed form: a wavefront per piece counts its kept bytes
//   exclusive_scan        of the kept bytes over the pieces (sum -> d_totals[0])
//   k_translate_offsets   per text: d_out_offsets[i] is the scan at its first piece; partial maxima of the lengths
//   k_translate_longest   the longest text -> d_totals[1]
//   k_translate_emit      a wavefront per piece: the kept, mapped bytes through the LDS stage of mrx_pieces.hpp
//   k_strip               a lane per text: (start, end)
// The lookup table is filled into LDS once per workgroup, from the kernel's arguments.  No atomics, no
// inline assembly, and no wavefront waits for another one.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_pieces.hpp"
#include "mrx_translate_bits.hpp"

namespace mrx {
namespace {

constexpr int kTrBlockDim = 256, kTrWaves = kTrBlockDim / 64;
constexpr unsigned kTrMaxGrid = 2048;   // 8 workgroups per CU; the kernels stride over what is left
constexpr int kTrParts = 1024;          // partial maxima of the longest text
constexpr int64_t kTrPieceMax = 1 << 20;

std::atomic<int64_t> g_tr_piece{0};
std::atomic<int64_t> g_tr_syncs{0};

int64_t tr_piece() {
  const int64_t pinned = g_tr_piece.load();
  return pinned > 0 ? pinned : kTranslatePiece;
}

// the plan's table, in LDS behind a barrier of the workgroup (every lane of it calls this once)
__device__ __forceinline__ const uint16_t* tr_lds_table(const TrPlan& P, uint16_t* lds) {
  for (int c = (int)threadIdx.x; c < 256; c += (int)blockDim.x) lds[c] = P.lut[c];
  __syncthreads();
  return lds;
}

// where the same-length form's region lies: CSR [offsets[0], offsets[n]) of both buffers, read on the device; fixed
// pitch [0, bytes)
struct TrRegion {
  const uint8_t* src;
  uint8_t* dst;
  const int64_t* offsets;
  int64_t n, bytes, out_cap;
};

__global__ __launch_bounds__(kTrBlockDim) void k_translate_map(const TrPlan P, const TrRegion R) {
  __shared__ uint16_t lds[256];
  const uint16_t* lut = tr_lds_table(P, lds);
  int64_t a = 0, N = R.bytes;
  if (R.offsets) {
    a = R.offsets[0];
    N = R.offsets[R.n] - a;
    if (a < 0 || a + N > R.out_cap) return;   // (a capacity that the host could not check: nothing is written)
  }
  if (N <= 0) return;
  const uint8_t* src = R.src + a;
  uint8_t* dst = R.dst + a;
  const int64_t nblk = tr_map_blocks(dst, N);
  for (int64_t b = (int64_t)blockIdx.x * kTrBlockDim + threadIdx.x; b < nblk; b += (int64_t)gridDim.x * kTrBlockDim)
    tr_map_block(lut, src, dst, N, b);
}

__global__ __launch_bounds__(kTrBlockDim) void k_translate_count(const TrPlan P, const TextBatch B, int64_t n, const LinesPieces pc,
                                                                int64_t* __restrict__ kept) {
  __shared__ uint16_t lds[256];
  const uint16_t* lut = tr_lds_table(P, lds);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int64_t piece = (int64_t)blockIdx.x * kTrWaves + wave; piece < pc.npieces; piece += (int64_t)gridDim.x * kTrWaves) {
    const LinesJob job = lines_job(B, n, pc, piece);
    int kp = 0;
    for (int64_t q = job.p0 + 16 * lane; q < job.pend; q += kLinesRound) kp += lines_popc(tr_block(P.mode, lut, job.tp, job.L, q).keep);
    kp = wave_sum(kp);
    if (lane == 0) kept[piece] = kp;
  }
}

// out_offsets[i] = scan[first piece of text i]; the largest length of a workgroup's texts -> part[blockIdx.x]
__global__ __launch_bounds__(256) void k_translate_offsets(int64_t n, const LinesPieces pc, const int64_t* __restrict__ scan,
                                                           int64_t* __restrict__ out_offsets, int64_t* __restrict__ part) {
  __shared__ int64_t wmax[4];
  int64_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = pc.first ? pc.first[i] : i * pc.per_text, b = pc.first ? pc.first[i + 1] : a + pc.per_text;
    a = a < pc.npieces ? a : pc.npieces;   // (only offsets that break the contract put a text's pieces behind the scan)
    b = b < pc.npieces ? b : pc.npieces;
    out_offsets[i] = scan[a];
    if (i == n - 1) out_offsets[n] = scan[b];
    const int64_t len = scan[b] - scan[a];
    m = len > m ? len : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t y = __shfl_xor(m, off);
    m = y > m ? y : m;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) m = wmax[w] > m ? wmax[w] : m;
    part[blockIdx.x] = m;
  }
}
__global__ __launch_bounds__(64) void k_translate_longest(const int64_t* __restrict__ part, int nparts, int64_t* __restrict__ totals) {
  int64_t m = 0;
  for (int k = (int)threadIdx.x; k < nparts; k += 64) m = part[k] > m ? part[k] : m;
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t y = __shfl_xor(m, off);
    m = y > m ? y : m;
  }
  if (threadIdx.x == 0) totals[1] = m;
}

__shared__ g_u64x2 s_tr_stage[kTrWaves][kLinesStage / 16];

__global__ __launch_bounds__(kTrBlockDim) void k_translate_emit(const TrPlan P, const TextBatch B, int64_t n, const LinesPieces pc,
                                                               const int64_t* __restrict__ scan, const int64_t* __restrict__ totals,
                                                               uint8_t* out, int64_t out_cap) {
  __shared__ uint16_t lds[256];
  const uint16_t* lut = tr_lds_table(P, lds);
  const int64_t bytes = totals[0];
  if (bytes <= 0 || bytes > out_cap) return;   // no byte at all
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  g_u64x2* stage16 = s_tr_stage[wave];
  for (int64_t piece = (int64_t)blockIdx.x * kTrWaves + wave; piece < pc.npieces; piece += (int64_t)gridDim.x * kTrWaves) {
    const LinesJob job = lines_job(B, n, pc, piece);
    const bool has = job.pend > job.p0;
    LinesStage st = lines_stage_open(has, out, has ? scan[piece] : 0);
    for (int64_t q0 = job.p0; q0 < job.pend; q0 += kLinesRound) {
      const int64_t q = q0 + 16 * lane;
      TrBlock b{0, 0};
      if (q < job.pend) b = tr_block(P.mode, lut, job.tp, job.L, q);
      const int mine = lines_popc(b.keep);
      int inc = mine;
      for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
      }
      lines_stage_round(st, stage16, lane, b.bytes, b.keep, inc - mine, __shfl(inc, 63));
    }
    lines_stage_close(st, stage16, lane);
  }
}

struct StripOut {
  int32_t* rows;
  int64_t* prefix;
};
__global__ __launch_bounds__(kTrBlockDim) void k_strip(const TrPlan P, const TextBatch B, int64_t n, uint32_t flags, const StripOut O) {
  __shared__ uint16_t lds[256];
  const uint16_t* lut = tr_lds_table(P, lds);
  for (int64_t i = (int64_t)blockIdx.x * kTrBlockDim + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTrBlockDim) {
    int64_t L, s, e;
    const uint8_t* tp = lines_text(B, i, &L);
    strip_text(lut, tp, L, flags, &s, &e);
    *(int2*)(O.rows + 2 * i) = make_int2((int)s, (int)e);
    if (O.prefix) {
      O.prefix[i] = i;
      if (i == n - 1) O.prefix[n] = n;
    }
  }
}

struct TranslateCall {
  const uint8_t* table;
  const uint8_t* del;
  const uint8_t* sq;
  uint8_t* d_out_data;
  int64_t out_cap;
  int64_t* d_out_offsets;
  int64_t* d_totals;
  int64_t* totals;
  void* stream;
};

// argument errors: nothing has touched the device when one of them returns.  The options, which the host hooks share ...
int translate_check_options(const uint8_t* del, const uint8_t* sq, int64_t n, int64_t out_cap) {
  if (tr_any(del) && tr_any(sq)) return internal_fail(MRX_E_ARGUMENT, "delete and squeeze in one call: translate twice");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "out_cap must be >= 0");
  return MRX_OK;
}
// ... and the batch and the pointers of a device call
int translate_check(const TextBatch& b, BatchForm form, int64_t n, const TranslateCall& c) {
  if (int rc = translate_check_options(c.del, c.sq, n, c.out_cap)) return rc;
  if (int rc = check_batch(b, form)) return rc;
  const bool packed = tr_any(c.del) || tr_any(c.sq);
  if ((packed && (!c.d_out_offsets || !c.d_totals)) || (c.out_cap > 0 && !c.d_out_data)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  return MRX_OK;
}

// the same-length form.  known_total: what the host knows of a CSR batch's last offset (< 0: read back)
int translate_map(const TrPlan& P, const TextBatch& b, int64_t n, int64_t known_total, const TranslateCall& c) {
  hipStream_t hs = (hipStream_t)c.stream;
  TrRegion R{b.data, c.d_out_data, b.offsets, n, 0, c.out_cap};
  int64_t end = known_total;   // the last byte of the region, in both buffers
  if (b.offsets) {
    if (end < 0) {
      int64_t ends[2] = {0, 0};
      MRX_HIP_TRY(hipMemcpyAsync(&ends[0], b.offsets, sizeof(int64_t), hipMemcpyDeviceToHost, hs));
      MRX_HIP_TRY(hipMemcpyAsync(&ends[1], b.offsets + n, sizeof(int64_t), hipMemcpyDeviceToHost, hs));
      MRX_HIP_TRY(hipStreamSynchronize(hs));
      ++g_tr_syncs;
      if (ends[1] < ends[0] || ends[0] < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
      end = ends[1];
    }
  } else {
    end = R.bytes = (n - 1) * b.stride + b.pitch_longest();
  }
  if (end > c.out_cap) return internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(end));
  set_last_kernel("k_translate_map");
  if (end <= 0) return MRX_OK;
  const unsigned grid = grid_for(end / 16 + 2, kTrBlockDim, kTrMaxGrid);
  void* timer = scan_timer_begin(c.stream);
  hipLaunchKernelGGL(k_translate_map, dim3(grid), dim3(kTrBlockDim), 0, hs, P, R);
  MRX_HIP_TRY(hipGetLastError());
  scan_timer_end(timer);
  return MRX_OK;
}

int translate_run(const TextBatch& b, BatchForm form, int64_t n, int64_t known_total, const TranslateCall& c) {
  if (int rc = translate_check(b, form, n, c)) return rc;
  hipStream_t hs = (hipStream_t)c.stream;
  TrPlan P;
  tr_plan(c.table, c.del, c.sq, nullptr, &P);
  const PackedDest o{nullptr, c.d_out_offsets, c.d_out_data, c.out_cap, c.d_totals, c.totals, c.stream};
  if (P.mode == TR_MAP) {
    if (n == 0) {
      set_last_kernel("k_translate_map");
      return MRX_OK;
    }
    return translate_map(P, b, n, known_total, c);
  }
  if (n == 0) {
    set_last_kernel("k_translate_emit");
    return packed_empty(o);
  }
  ScratchScope scope_(c.stream);
  LinesPieces pc{tr_piece(), 0, nullptr, 0};
  int64_t* dummy = (int64_t*)scratch_get(sizeof(int64_t), c.stream);   // the sum of the scan that nobody reads
  if (!dummy) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  if (int rc = lines_pieces_setup(b, n, known_total, dummy, g_tr_syncs, c.stream, &pc)) return rc;
  const size_t np = (size_t)pc.npieces, i64 = sizeof(int64_t);
  int64_t* kept = (int64_t*)scratch_get(i64 * np, c.stream);
  int64_t* scan = (int64_t*)scratch_get(i64 * (np + 1), c.stream);
  int64_t* part = (int64_t*)scratch_get(i64 * kTrParts, c.stream);
  if (!kept || !scan || !part) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  void* timer = scan_timer_begin(c.stream);
  const int rc = [&]() -> int {
    const unsigned grid = grid_for(pc.npieces, kTrWaves, kTrMaxGrid), tgrid = grid_for(n, 256, kTrParts);
    hipLaunchKernelGGL(k_translate_count, dim3(grid), dim3(kTrBlockDim), 0, hs, P, b, n, pc, kept);
    MRX_HIP_TRY(hipGetLastError());
    if (int rc = exclusive_scan(kept, pc.npieces, scan, c.d_totals, c.stream)) return rc;
    hipLaunchKernelGGL(k_translate_offsets, dim3(tgrid), dim3(256), 0, hs, n, pc, scan, c.d_out_offsets, part);
    hipLaunchKernelGGL(k_translate_longest, dim3(1), dim3(64), 0, hs, part, (int)tgrid, c.d_totals);
    MRX_HIP_TRY(hipGetLastError());
    if (c.out_cap > 0) hipLaunchKernelGGL(k_translate_emit, dim3(grid), dim3(kTrBlockDim), 0, hs, P, b, n, pc, scan, c.d_totals, c.d_out_data, c.out_cap);
    MRX_HIP_TRY(hipGetLastError());
    return MRX_OK;
  }();
  scan_timer_end(timer);
  if (rc) return rc;
  set_last_kernel("k_translate_emit");
  if (!c.totals) return MRX_OK;
  // (packed_verdict reads {rows, bytes}: these totals are {bytes, longest text})
  MRX_HIP_TRY(hipMemcpyAsync(c.totals, c.d_totals, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));
  ++g_tr_syncs;
  if (c.totals[0] > c.out_cap) return internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(c.totals[0]));
  return MRX_OK;
}

struct StripCall {
  const uint8_t* set;
  uint32_t flags;
  int32_t* d_rows;
  int64_t* d_prefix;
  void* stream;
};
const uint8_t kWhitespace[32] = {0x00, 0x3e, 0, 0, 0x01};   // 0x09 .. 0x0d and 0x20, as fields

int strip_check_options(uint32_t flags, int64_t n) {
  if ((flags & ~(uint32_t)(MRX_STRIP_LEFT | MRX_STRIP_RIGHT)) || !flags)
    return internal_fail(MRX_E_ARGUMENT, "flags must be MRX_STRIP_LEFT, MRX_STRIP_RIGHT or both");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  return MRX_OK;
}
void strip_plan(const uint8_t* set, TrPlan* P) {
  tr_plan(nullptr, nullptr, nullptr, set ? set : kWhitespace, P);
  P->mode = TR_STRIP;   // (an empty set strips nothing)
}
int strip_run(const TextBatch& b, BatchForm form, int64_t n, const StripCall& c) {
  if (int rc = strip_check_options(c.flags, n)) return rc;
  if (int rc = check_batch(b, form)) return rc;
  if (!c.d_rows) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if ((uintptr_t)c.d_rows & 7) return internal_fail(MRX_E_ARGUMENT, "d_rows must be 8-byte aligned");
  set_last_kernel("k_strip");
  if (n == 0) return MRX_OK;
  TrPlan P;
  strip_plan(c.set, &P);
  hipStream_t hs = (hipStream_t)c.stream;
  hipLaunchKernelGGL(k_strip, dim3(grid_for(n, kTrBlockDim, kTrMaxGrid)), dim3(kTrBlockDim), 0, hs, P, b, n, c.flags, StripOut{c.d_rows, c.d_prefix});
  MRX_HIP_TRY(hipGetLastError());
  return MRX_OK;
}

// the texts of a host hook at their own alignment inside a buffer that owns the aligned words around them; everything
// else in it is `fill`
struct HostCopy {
  std::vector<g_u64x2> room;
  std::vector<int64_t> rel;
  uint8_t* at = nullptr;
  int64_t bytes = 0;
  int build(const uint8_t* data, const int64_t* offsets, int64_t n, uint8_t fill) {
    if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
    if (!offsets) return internal_fail(MRX_E_ARGUMENT, "null argument");
    for (int64_t i = 0; i < n; ++i)
      if (offsets[i + 1] < offsets[i]) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
    bytes = n > 0 ? offsets[n] - offsets[0] : 0;
    if (bytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
    const size_t skew = n > 0 && data ? (size_t)((uintptr_t)(data + offsets[0]) & 15) : 0;
    room.resize((size_t)bytes / 16 + 3);
    memset(room.data(), fill, room.size() * 16);
    at = (uint8_t*)room.data() + skew;
    if (bytes > 0) memcpy(at, data + offsets[0], (size_t)bytes);
    rel.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i <= n && n > 0; ++i) rel[(size_t)i] = offsets[i] - offsets[0];
    return MRX_OK;
  }
};

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_translate_dev(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set, const uint8_t* d_data,
                      const int64_t* d_offsets, int64_t n, uint8_t* d_out_data, int64_t out_cap, int64_t* d_out_offsets,
                      int64_t* d_totals, int64_t* totals, void* stream) {
  return translate_run(csr(d_data, d_offsets), BATCH_CSR, n, -1,
                       TranslateCall{table, delete_set, squeeze_set, d_out_data, out_cap, d_out_offsets, d_totals, totals, stream});
}
int mrx_translate_known_dev(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set, const uint8_t* d_data,
                            const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len, uint8_t* d_out_data,
                            int64_t out_cap, int64_t* d_out_offsets, int64_t* d_totals, int64_t* totals, void* stream) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return translate_run(csr(d_data, d_offsets), BATCH_CSR, n, end_offset,
                       TranslateCall{table, delete_set, squeeze_set, d_out_data, out_cap, d_out_offsets, d_totals, totals, stream});
}
int mrx_translate_strided_dev(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set, const uint8_t* d_data,
                              int64_t stride, const int32_t* d_lens, int32_t len, int64_t n, uint8_t* d_out_data, int64_t out_cap,
                              int64_t* d_out_offsets, int64_t* d_totals, int64_t* totals, void* stream) {
  return translate_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1,
                       TranslateCall{table, delete_set, squeeze_set, d_out_data, out_cap, d_out_offsets, d_totals, totals, stream});
}

int mrx_strip_dev(const uint8_t* set, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int32_t* d_rows,
                  int64_t* d_prefix, void* stream) {
  return strip_run(csr(d_data, d_offsets), BATCH_CSR, n, StripCall{set, flags, d_rows, d_prefix, stream});
}
int mrx_strip_known_dev(const uint8_t* set, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t end_offset, int64_t max_text_len, int32_t* d_rows, int64_t* d_prefix, void* stream) {
  if (end_offset < 0 || max_text_len < 0) return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must be >= 0");
  return strip_run(csr(d_data, d_offsets), BATCH_CSR, n, StripCall{set, flags, d_rows, d_prefix, stream});
}
int mrx_strip_strided_dev(const uint8_t* set, uint32_t flags, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                          int32_t len, int64_t n, int32_t* d_rows, int64_t* d_prefix, void* stream) {
  return strip_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n, StripCall{set, flags, d_rows, d_prefix, stream});
}

// host buffers: argument errors before any device work, as the _dev entry points
int mrx_translate_batch(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set, const uint8_t* data,
                        const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap,
                        int64_t* totals) {
  if (int rc = translate_check_options(delete_set, squeeze_set, n, out_cap)) return rc;
  if (!offsets || !out_offsets || (out_cap > 0 && !out_data)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  DevBatch b; DevBuf<int64_t> oo, dt; DevBuf<uint8_t> od;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  const bool packed = tr_any(delete_set) || tr_any(squeeze_set);
  if (!packed) {   // the same layout: the offsets relative to the first text, the totals from the host's own offsets
    if (b.nbytes > out_cap) {
      if (totals) totals[0] = b.nbytes, totals[1] = b.longest;
      memcpy(out_offsets, b.rel.data(), sizeof(int64_t) * ((size_t)n + 1));
      return internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(b.nbytes));
    }
  }
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = oo.alloc((size_t)n + 1)) return rc;
  if (int rc = dt.alloc(2)) return rc;
  if (int rc = od.alloc((size_t)out_cap)) return rc;
  int64_t tot[2] = {b.nbytes, b.longest};
  const int rc = mrx_translate_known_dev(table, delete_set, squeeze_set, b.data, b.offsets, n, b.nbytes, b.longest, od.p, out_cap,
                                         oo.p, dt.p, packed ? tot : nullptr, nullptr);
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  if (totals) memcpy(totals, tot, sizeof tot);
  if (packed) MRX_HIP_TRY(hipMemcpy(out_offsets, oo.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost));
  else memcpy(out_offsets, b.rel.data(), sizeof(int64_t) * ((size_t)n + 1));
  if (rc == MRX_OK && tot[0] > 0) MRX_HIP_TRY(hipMemcpy(out_data, od.p, (size_t)tot[0], hipMemcpyDeviceToHost));
  return rc;
}

int mrx_strip_batch(const uint8_t* set, uint32_t flags, const uint8_t* data, const int64_t* offsets, int64_t n, int32_t* rows,
                    int64_t* prefix) {
  if (int rc = strip_check_options(flags, n)) return rc;
  if (!offsets || !rows) return internal_fail(MRX_E_ARGUMENT, "null argument");
  DevBatch b; DevBuf<int32_t> dr; DevBuf<int64_t> dp;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n == 0) return MRX_OK;
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = dr.alloc((size_t)n * 2)) return rc;
  if (prefix) if (int rc = dp.alloc((size_t)n + 1)) return rc;
  if (int rc = mrx_strip_known_dev(set, flags, b.data, b.offsets, n, b.nbytes, b.longest, dr.p, prefix ? dp.p : nullptr, nullptr)) return rc;
  MRX_HIP_TRY(hipMemcpy(rows, dr.p, sizeof(int32_t) * (size_t)n * 2, hipMemcpyDeviceToHost));
  if (prefix) MRX_HIP_TRY(hipMemcpy(prefix, dp.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost));
  return MRX_OK;
}

int64_t mrx_debug_translate_piece(int64_t bytes) {
  if (bytes >= 0) {
    int64_t P = (bytes + kLinesRound - 1) / kLinesRound * kLinesRound;
    g_tr_piece.store(P > kTrPieceMax ? kTrPieceMax : P);
  }
  return tr_piece();
}
int64_t mrx_debug_translate_syncs(void) { return g_tr_syncs.load(); }

int mrx_debug_translate_host(const uint8_t* table, const uint8_t* delete_set, const uint8_t* squeeze_set, const uint8_t* data,
                             const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap,
                             int64_t* totals) {
  if (int rc = translate_check_options(delete_set, squeeze_set, n, out_cap)) return rc;
  if (!out_offsets || (out_cap > 0 && !out_data)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  HostCopy in;
  // (what lies around the texts would change the result if the walk took it for text: a member of the sets)
  uint8_t fill = ' ';
  for (int c = 0; c < 256; ++c)
    if (tr_bit(delete_set, c) || tr_bit(squeeze_set, c)) fill = (uint8_t)c;
  if (int rc = in.build(data, offsets, n, fill)) return rc;
  TrPlan P;
  tr_plan(table, delete_set, squeeze_set, nullptr, &P);
  int64_t tot[2] = {0, 0};
  if (P.mode == TR_MAP) {
    tot[0] = in.bytes;
    for (int64_t i = 0; i < n; ++i) tot[1] = std::max(tot[1], in.rel[(size_t)i + 1] - in.rel[(size_t)i]);
    memcpy(out_offsets, in.rel.data(), sizeof(int64_t) * ((size_t)n + 1));
    if (tot[0] <= out_cap) translate_map_host(P, in.at, out_data, in.bytes);
  } else {
    translate_host(P, in.at, in.rel.data(), n, tr_piece(), TrHostOut{out_offsets, out_data, out_cap, tot});
  }
  if (totals) memcpy(totals, tot, sizeof tot);
  if (tot[0] > out_cap) return internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(tot[0]));
  return MRX_OK;
}

int mrx_debug_strip_host(const uint8_t* set, uint32_t flags, const uint8_t* data, const int64_t* offsets, int64_t n, int32_t* rows,
                         int64_t* prefix) {
  if (int rc = strip_check_options(flags, n)) return rc;
  if (!rows) return internal_fail(MRX_E_ARGUMENT, "null argument");
  HostCopy in;
  if (int rc = in.build(data, offsets, n, 'q')) return rc;
  TrPlan P;
  strip_plan(set, &P);
  strip_host(P, in.at, in.rel.data(), n, flags, rows);
  for (int64_t i = 0; prefix && i <= n; ++i) prefix[i] = i;
  return MRX_OK;
}

}  // extern "C"
