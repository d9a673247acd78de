// Keywords, leftmost and sub (include/mrx.h, "keywords: leftmost-longest matches and replacement"): the launches and the
// entry points.  The walk back, the selection, the rows and the block fill are in mrx_kw_sub_bits.hpp; the handle, the
// LDS tier and the pieces are those of mrx_keywords.hip (mrx_kw_dev.hpp).
//
//   k_kw_cand_count   a lane walks a piece back through the reversed automaton: its candidate count and reach[piece]
//   exclusive_scan    over the pieces' counts; the ONE synchronisation in front of the end: the candidate total C
//   k_kw_cand_emit    walks the pieces that have candidates again and writes them, ascending by start
//   k_kw_sub_select   a lane per piece: the chain from the piece's first head (mrx_kw_sub_bits.hpp)
//   k_kw_sub_selcount a lane per piece: its selected candidates; exclusive_scan: their ranks
//   k_kw_sub_text     per text: the kept matches (all, or `count`), d_nsub; exclusive_scan: kb[n + 1], which is
//                     leftmost's d_text_prefix
//   leftmost          k_kw_sub_rows<false>: the kept matches at kb[text] + rank, clamped at span_cap
//   sub               k_kw_sub_tail and k_kw_sub_rows<true> write the 2 K + n rows (length, source address),
//                     exclusive_scan gives their CSR over the output, k_kw_sub_offsets d_out_offsets and the longest
//                     output text, k_kw_sub_gather the bytes: extract's block walk with a source address per row
// No memory atomics and no inline assembly: every flag, row and byte has exactly one writer.
// Scratch: 13 bytes per candidate, 24 per row (2 C + n rows at most), 36 per piece, 16 per text, and the scans' block sums.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_gather_bits.hpp"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_kw_dev.hpp"
#include "mrx_kw_sub_bits.hpp"

namespace mrx {
namespace {

constexpr int kSubBlock = 256;
constexpr unsigned kSubMaxGrid = 2048;
constexpr int kSubParts = 1024;   // partial maxima of the longest output text

__device__ __forceinline__ KwBackJob kw_piece_back_job(const TextBatch& B, int64_t n, const KwPieces& pc, int32_t lmax, int64_t piece) {
  int64_t i, lp;
  if (!kw_piece_text(pc, n, piece, &i, &lp)) return kw_no_back_job();
  int32_t L = 0;
  const uint8_t* tp = B.text(i, &L);
  return kw_back_job(tp, L, lp, pc.P, lmax);
}
// the first piece of text i (i <= n), clamped as k_kw_text clamps it
__device__ __forceinline__ int64_t kw_first_piece(const KwPieces& pc, int64_t i) {
  const int64_t a = pc.first ? pc.first[i] : i * pc.per_text;
  return a < pc.npieces ? a : pc.npieces;
}

__global__ __launch_bounds__(kKwBlock) void k_kw_cand_count(const TextBatch B, int64_t n, const KwView V, const KwPieces pc,
                                                            int64_t* __restrict__ cnt, int32_t* __restrict__ reach) {
  const KwDevTab tab = kw_stage_tier(V);
  const int64_t nthreads = (int64_t)gridDim.x * kKwBlock;
  for (int64_t piece = (int64_t)blockIdx.x * kKwBlock + threadIdx.x; piece < pc.npieces; piece += nthreads) {
    KwCandCount sink{V.meta, 0, 0};
    kw_walk_back(tab, kw_piece_back_job(B, n, pc, V.lmax, piece), sink);
    cnt[piece] = sink.cnt;
    reach[piece] = sink.reach;
  }
}
__global__ __launch_bounds__(kKwBlock) void k_kw_cand_emit(const TextBatch B, int64_t n, const KwView V, const KwPieces pc,
                                                           const int64_t* __restrict__ scan, const KwCands c) {
  const KwDevTab tab = kw_stage_tier(V);
  const int64_t nthreads = (int64_t)gridDim.x * kKwBlock;
  for (int64_t piece = (int64_t)blockIdx.x * kKwBlock + threadIdx.x; piece < pc.npieces; piece += nthreads) {
    const int64_t a = scan[piece], b = scan[piece + 1];
    if (a == b) continue;   // (a piece without candidates is not walked again)
    KwCandEmit sink{V.meta, c, b - 1};
    kw_walk_back(tab, kw_piece_back_job(B, n, pc, V.lmax, piece), sink);
  }
}

__global__ __launch_bounds__(kSubBlock) void k_kw_sub_select(int64_t n, const KwPieces pc, const int64_t* __restrict__ scan,
                                                             const int32_t* __restrict__ reach, const KwCands c, int64_t back) {
  const int64_t nthreads = (int64_t)gridDim.x * kSubBlock;
  for (int64_t piece = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; piece < pc.npieces; piece += nthreads) {
    if (scan[piece] == scan[piece + 1]) continue;
    int64_t i, lp;
    if (!kw_piece_text(pc, n, piece, &i, &lp)) continue;
    kw_sub_select(c, scan, reach, piece, lp, scan[kw_first_piece(pc, i + 1)], back);
  }
}
__global__ __launch_bounds__(kSubBlock) void k_kw_sub_selcount(int64_t npieces, const int64_t* __restrict__ scan,
                                                               const uint8_t* __restrict__ sel, int64_t* __restrict__ selcnt) {
  const int64_t nthreads = (int64_t)gridDim.x * kSubBlock;
  for (int64_t piece = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; piece < npieces; piece += nthreads)
    selcnt[piece] = kw_sub_selected(sel, scan[piece], scan[piece + 1]);
}
__global__ __launch_bounds__(kSubBlock) void k_kw_sub_text(int64_t n, const KwPieces pc, const int64_t* __restrict__ sscan,
                                                           int64_t count, int64_t* __restrict__ kept, int32_t* __restrict__ nsub) {
  for (int64_t i = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSubBlock) {
    const int64_t k = kw_sub_kept(sscan[kw_first_piece(pc, i + 1)] - sscan[kw_first_piece(pc, i)], count);
    kept[i] = k;
    if (nsub) nsub[i] = (int32_t)k;
  }
}
// a text without a kept match is its tail row
__global__ __launch_bounds__(kSubBlock) void k_kw_sub_tail(const TextBatch B, int64_t n, const int64_t* __restrict__ kb,
                                                           const KwSegs S) {
  for (int64_t i = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSubBlock) {
    if (kb[i + 1] != kb[i]) continue;
    int32_t L = 0;
    const uint8_t* tp = B.text(i, &L);
    S.len[2 * kb[i] + i] = L;
    S.src[2 * kb[i] + i] = tp;
  }
}
template <bool SUB>
__global__ __launch_bounds__(kSubBlock) void k_kw_sub_rows(const TextBatch B, int64_t n, const KwPieces pc,
                                                           const int64_t* __restrict__ scan, const int64_t* __restrict__ sscan,
                                                           const int64_t* __restrict__ kb, const KwCands c, const KwRepl R,
                                                           const KwSegs S, const KwSpansOut O) {
  const int64_t nthreads = (int64_t)gridDim.x * kSubBlock;
  for (int64_t piece = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; piece < pc.npieces; piece += nthreads) {
    if (sscan[piece] == sscan[piece + 1]) continue;   // nothing selected here
    int64_t i, lp;
    if (!kw_piece_text(pc, n, piece, &i, &lp)) continue;
    const int64_t f = kw_first_piece(pc, i);
    int32_t L = 0;
    const uint8_t* tp = B.text(i, &L);
    kw_sub_rows<SUB>(c, scan[piece], scan[piece + 1], scan[f], sscan[piece] - sscan[f], kb[i], kb[i + 1] - kb[i], i, tp, L, R, S, O);
  }
}
// out_offsets[i] = the output position of text i's first row; the largest length of a workgroup's texts -> part[blockIdx.x]
__global__ __launch_bounds__(kSubBlock) void k_kw_sub_offsets(int64_t n, const int64_t* __restrict__ kb,
                                                              const int64_t* __restrict__ segoff, int64_t* __restrict__ out_offsets,
                                                              int64_t* __restrict__ part) {
  __shared__ int64_t wmax[kSubBlock / 64];
  int64_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * kSubBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSubBlock) {
    const int64_t a = segoff[2 * kb[i] + i], b = segoff[2 * kb[i + 1] + i + 1];
    out_offsets[i] = a;
    if (i == n - 1) out_offsets[n] = b;
    m = b - a > m ? b - a : m;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t y = __shfl_xor(m, off);
    m = y > m ? y : m;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kSubBlock / 64; ++w) m = wmax[w] > m ? wmax[w] : m;
    part[blockIdx.x] = m;
  }
}
// totals = {output bytes (the scan's sum, already there), longest output text, replacements}
__global__ __launch_bounds__(64) void k_kw_sub_totals(const int64_t* __restrict__ part, int nparts, const int64_t* __restrict__ kb,
                                                      int64_t n, int64_t* __restrict__ totals) {
  int64_t m = 0;
  for (int k = (int)threadIdx.x; k < nparts; k += 64) m = part[k] > m ? part[k] : m;
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t y = __shfl_xor(m, off);
    m = y > m ? y : m;
  }
  if (threadIdx.x == 0) {
    totals[1] = m;
    totals[2] = kb[n];
  }
}

struct SubOut {
  const int64_t* segoff;      // [rows + 1]
  const uint8_t* const* src;  // [rows]
  const int64_t* kb;          // [n + 1]
  int64_t n;
  const int64_t* totals;      // {bytes, ...}
  uint8_t* out;
  int64_t out_cap;
};
__global__ __launch_bounds__(kSubBlock) void k_kw_sub_gather(const SubOut O) {
  const int64_t bytes = O.totals[0], rows = 2 * O.kb[O.n] + O.n;
  if (bytes <= 0 || bytes > O.out_cap) return;   // nothing is written when the output does not fit
  gather_blocks<kSubBlock>(O.out, bytes, O.segoff, rows, [&](int64_t r, int64_t hi, int64_t p0, int64_t pos, int64_t endp) {
    return kw_sub_fill(O.segoff, O.src, r, hi, p0, pos, endp);
  });
}

// the automaton of the reversed entries, built and uploaded once per handle
int kw_reversed(const mrx_kw* k, void* st) {
  std::call_once(k->rev_once, [&] {
    KwAutomaton A;
    k->rev_rc = kw_build_reversed(k->entry_data.data(), k->entry_off.data(), k->m, k->flags, &A, &k->rev_err);
    if (k->rev_rc) {
      k->rev_err = "leftmost / sub: the reversed entries: " + k->rev_err;
      return;
    }
    k->rev_rc = kw_upload_tables(A, st, &k->rev);
    if (!k->rev_rc && hipStreamSynchronize((hipStream_t)st) != hipSuccess) k->rev_rc = MRX_E_NO_DEVICE;
    if (k->rev_rc) k->rev_err = "leftmost / sub: the upload of the reversed automaton failed";
  });
  if (k->rev_rc) return internal_fail(k->rev_rc, k->rev_err);
  return MRX_OK;
}

// what the two operations share up to the kept matches of every text
struct SubRun {
  KwPieces pc;
  int64_t C = 0;              // candidates
  int64_t* scan = nullptr;    // [npieces + 1] of the candidates
  int64_t* sscan = nullptr;   // [npieces + 1] of the selected ones
  KwCands c{};
  unsigned pgrid = 1;         // a lane per piece, kSubBlock lanes a workgroup
};
// kb[n + 1] (the caller's: leftmost's d_text_prefix, or scratch) and *d_kept_total = kb[n]
int sub_select(const mrx_kw* k, const TextBatch& b, int64_t n, int64_t known_total, int64_t known_max, int64_t count,
               int32_t* d_nsub, int64_t* kb, int64_t* d_kept_total, SubRun& r, void* st) {
  hipStream_t hs = (hipStream_t)st;
  if (int rc = kw_reversed(k, st)) return rc;
  KwPieces& pc = r.pc;
  if (int rc = kw_plan_pieces(k->lmax, b, n, known_total, known_max, pc, st)) return rc;
  const KwView view = kw_view(k->rev, k->lmax);
  const unsigned wgrid = grid_for(pc.npieces, kKwBlock, kKwMaxGrid);
  r.pgrid = grid_for(pc.npieces, kSubBlock, kSubMaxGrid);
  int64_t* cnt = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)pc.npieces, st);
  int32_t* reach = (int32_t*)scratch_get(sizeof(int32_t) * (size_t)pc.npieces, st);
  r.scan = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(pc.npieces + 1), st);
  r.sscan = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(pc.npieces + 1), st);
  int64_t* kept = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, st);
  int64_t* d_total = (int64_t*)scratch_get(sizeof(int64_t) * 2, st);
  if (!cnt || !reach || !r.scan || !r.sscan || !kept || !d_total) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  void* timer = scan_timer_begin(st);
  hipLaunchKernelGGL(k_kw_cand_count, dim3(wgrid), dim3(kKwBlock), 0, hs, b, n, view, pc, cnt, reach);
  scan_timer_end(timer);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(cnt, pc.npieces, r.scan, d_total, st)) return rc;
  MRX_HIP_TRY(hipMemcpyAsync(&r.C, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));   // the candidate total sizes the scratch
  const size_t cap = (size_t)(r.C > 0 ? r.C : 1);
  r.c.start = (int32_t*)scratch_get(sizeof(int32_t) * cap, st);
  r.c.end = (int32_t*)scratch_get(sizeof(int32_t) * cap, st);
  r.c.entry = (int32_t*)scratch_get(sizeof(int32_t) * cap, st);
  r.c.sel = (uint8_t*)scratch_get(cap, st);
  if (!r.c.start || !r.c.end || !r.c.entry || !r.c.sel) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  if (r.C > 0) {
    const int64_t warm = k->lmax > 0 ? k->lmax - 1 : 0;
    hipLaunchKernelGGL(k_kw_cand_emit, dim3(wgrid), dim3(kKwBlock), 0, hs, b, n, view, pc, r.scan, r.c);
    MRX_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_kw_sub_select, dim3(r.pgrid), dim3(kSubBlock), 0, hs, n, pc, r.scan, reach, r.c, (warm + pc.P - 1) / pc.P);
    MRX_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_kw_sub_selcount, dim3(r.pgrid), dim3(kSubBlock), 0, hs, pc.npieces, r.scan, r.c.sel, cnt);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(cnt, pc.npieces, r.sscan, d_total + 1, st)) return rc;
  hipLaunchKernelGGL(k_kw_sub_text, dim3(grid_for(n, kSubBlock, kSubMaxGrid)), dim3(kSubBlock), 0, hs, n, pc, r.sscan, count, kept, d_nsub);
  MRX_HIP_TRY(hipGetLastError());
  return exclusive_scan(kept, n, kb, d_kept_total, st);
}

int kw_leftmost(const mrx_kw* k, int64_t count, const TextBatch& b, BatchForm form, int64_t n, int64_t known_total,
                int64_t known_max, int64_t* d_text_prefix, int32_t* d_entries, int32_t* d_spans, int64_t span_cap, int64_t* total,
                void* st) {
  if (!k) return internal_fail(MRX_E_ARGUMENT, "null keyword set");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (count < 0) return internal_fail(MRX_E_ARGUMENT, "count must be >= 0");
  if (span_cap < 0) return internal_fail(MRX_E_ARGUMENT, "span_cap must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (!d_text_prefix || (n > 0 && span_cap > 0 && (!d_entries || !d_spans))) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if ((uintptr_t)d_spans & 7) return internal_fail(MRX_E_ARGUMENT, "d_spans must be 8-byte aligned");
  hipStream_t hs = (hipStream_t)st;
  if (total) *total = 0;
  if (n == 0) {
    MRX_HIP_TRY(hipMemsetAsync(d_text_prefix, 0, sizeof(int64_t), hs));
    return MRX_OK;
  }
  ScratchScope scope_(st);
  int64_t* d_k = (int64_t*)scratch_get(sizeof(int64_t), st);
  if (!d_k) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  SubRun r;
  if (int rc = sub_select(k, b, n, known_total, known_max, count, nullptr, d_text_prefix, d_k, r, st)) return rc;
  if (r.C > 0 && span_cap > 0) {
    hipLaunchKernelGGL(k_kw_sub_rows<false>, dim3(r.pgrid), dim3(kSubBlock), 0, hs, b, n, r.pc, r.scan, r.sscan, d_text_prefix, r.c,
                       KwRepl{nullptr, nullptr, 1}, KwSegs{nullptr, nullptr}, KwSpansOut{d_entries, d_spans, span_cap});
    MRX_HIP_TRY(hipGetLastError());
  }
  set_last_kernel("k_kw_sub_select");
  int64_t tot = 0;
  MRX_HIP_TRY(hipMemcpyAsync(&tot, d_k, sizeof(int64_t), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));   // the read-back at the end: the total
  if (total) *total = tot;
  if (tot > span_cap) return internal_fail(MRX_E_CAPACITY, "span buffer too small: need " + std::to_string(tot));
  return MRX_OK;
}

struct SubArgs {
  const uint8_t* d_repl_data;
  const int64_t* d_repl_offsets;
  int64_t r, count;
  int64_t* d_out_offsets;
  uint8_t* d_out_data;
  int64_t out_cap;
  int32_t* d_nsub;
  int64_t* d_totals;
  int64_t* totals;
  void* stream;
};

int kw_sub(const mrx_kw* k, const TextBatch& b, BatchForm form, int64_t n, int64_t known_total, int64_t known_max, const SubArgs& a) {
  void* st = a.stream;
  if (!k) return internal_fail(MRX_E_ARGUMENT, "null keyword set");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (a.count < 0) return internal_fail(MRX_E_ARGUMENT, "count must be >= 0");
  if (a.r < 0) return internal_fail(MRX_E_ARGUMENT, "r must be >= 0");
  if (a.out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "out_cap must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (!a.d_out_offsets || (a.out_cap > 0 && !a.d_out_data) || (a.r > 0 && (!a.d_repl_data || !a.d_repl_offsets)))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (a.r != 1 && a.r != k->m)
    return internal_fail(MRX_E_ARGUMENT, "r must be 1 or the number of entries, " + std::to_string(k->m));
  hipStream_t hs = (hipStream_t)st;
  if (a.totals) a.totals[0] = a.totals[1] = a.totals[2] = 0;
  if (n == 0) {
    MRX_HIP_TRY(hipMemsetAsync(a.d_out_offsets, 0, sizeof(int64_t), hs));
    if (a.d_totals) MRX_HIP_TRY(hipMemsetAsync(a.d_totals, 0, 3 * sizeof(int64_t), hs));
    set_last_kernel("k_kw_sub_gather");
    return MRX_OK;
  }
  ScratchScope scope_(st);
  int64_t* kb = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), st);
  int64_t* d_totals = a.d_totals ? a.d_totals : (int64_t*)scratch_get(sizeof(int64_t) * 3, st);
  int64_t* part = (int64_t*)scratch_get(sizeof(int64_t) * kSubParts, st);
  if (!kb || !d_totals || !part) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  SubRun r;
  if (int rc = sub_select(k, b, n, known_total, known_max, a.count, a.d_nsub, kb, d_totals + 2, r, st)) return rc;
  const int64_t rows = 2 * r.C + n;   // 2 K + n are used, K <= C; the others keep the length 0
  KwSegs S;
  S.len = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)rows, st);
  S.src = (const uint8_t**)scratch_get(sizeof(const uint8_t*) * (size_t)rows, st);
  int64_t* segoff = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(rows + 1), st);
  if (!S.len || !S.src || !segoff) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  MRX_HIP_TRY(hipMemsetAsync(S.len, 0, sizeof(int64_t) * (size_t)rows, hs));
  const unsigned tgrid = grid_for(n, kSubBlock, kSubParts);
  hipLaunchKernelGGL(k_kw_sub_tail, dim3(tgrid), dim3(kSubBlock), 0, hs, b, n, kb, S);
  MRX_HIP_TRY(hipGetLastError());
  if (r.C > 0) {
    hipLaunchKernelGGL(k_kw_sub_rows<true>, dim3(r.pgrid), dim3(kSubBlock), 0, hs, b, n, r.pc, r.scan, r.sscan, kb, r.c,
                       KwRepl{a.d_repl_data, a.d_repl_offsets, a.r}, S, KwSpansOut{nullptr, nullptr, 0});
    MRX_HIP_TRY(hipGetLastError());
  }
  if (int rc = exclusive_scan(S.len, rows, segoff, d_totals, st)) return rc;
  hipLaunchKernelGGL(k_kw_sub_offsets, dim3(tgrid), dim3(kSubBlock), 0, hs, n, kb, segoff, a.d_out_offsets, part);
  MRX_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_kw_sub_totals, dim3(1), dim3(64), 0, hs, part, (int)tgrid, kb, n, d_totals);
  MRX_HIP_TRY(hipGetLastError());
  if (a.out_cap > 0) {   // (nothing fits a capacity of 0, and no empty output has a byte to move)
    const SubOut O{segoff, S.src, kb, n, d_totals, a.d_out_data, a.out_cap};
    hipLaunchKernelGGL(k_kw_sub_gather, dim3(grid_for(a.out_cap / 16 + 2, kSubBlock, kSubMaxGrid)), dim3(kSubBlock), 0, hs, O);
    MRX_HIP_TRY(hipGetLastError());
  }
  set_last_kernel("k_kw_sub_gather");
  if (!a.totals) return MRX_OK;
  MRX_HIP_TRY(hipMemcpyAsync(a.totals, d_totals, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));   // the read-back at the end: the totals
  if (a.totals[0] > a.out_cap) return internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(a.totals[0]));
  return MRX_OK;
}

// the texts of a hook at their own alignment inside a buffer that owns the aligned words around them
struct HostPlaced {
  std::vector<g_u64x2> room;
  std::vector<int64_t> rel;
  const uint8_t* p = nullptr;
  void place(const uint8_t* data, const int64_t* off, int64_t n) {
    const int64_t bytes = n > 0 ? off[n] - off[0] : 0;
    const size_t skew = n > 0 && data ? (size_t)((uintptr_t)(data + off[0]) & 15) : 0;
    room.assign((size_t)bytes / 16 + 3, g_u64x2{0, 0});
    uint8_t* copy = (uint8_t*)room.data() + skew;
    if (bytes > 0) memcpy(copy, data + off[0], (size_t)bytes);
    rel.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i <= n && n > 0; ++i) rel[(size_t)i] = off[i] - off[0];
    p = copy;
  }
};
int host_check_texts(const uint8_t* data, const int64_t* offsets, int64_t n) {
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (!offsets) return internal_fail(MRX_E_ARGUMENT, "null argument");
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (n > 0 && offsets[n] > offsets[0] && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  return MRX_OK;
}
int host_reversed(const uint8_t* entry_data, const int64_t* entry_offsets, int64_t m, uint32_t flags, KwAutomaton* A) {
  int dummy = 0;
  if (int rc = kw_check_build(m, flags, entry_offsets, &dummy)) return rc;
  if (m > 0 && entry_offsets[m] > entry_offsets[0] && !entry_data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  std::string err;
  if (int rc = kw_build_reversed(entry_data, entry_offsets, m, flags, A, &err)) return internal_fail(rc, err);
  return MRX_OK;
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_kw_leftmost_dev(const mrx_kw* k, int64_t count, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t* d_text_prefix, int32_t* d_entries, int32_t* d_spans, int64_t span_cap, int64_t* total, void* stream) {
  return kw_leftmost(k, count, csr(d_data, d_offsets), BATCH_CSR, n, -1, -1, d_text_prefix, d_entries, d_spans, span_cap, total, stream);
}
int mrx_kw_leftmost_known_dev(const mrx_kw* k, int64_t count, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                              int64_t end_offset, int64_t max_text_len, int64_t* d_text_prefix, int32_t* d_entries,
                              int32_t* d_spans, int64_t span_cap, int64_t* total, void* stream) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return kw_leftmost(k, count, csr(d_data, d_offsets), BATCH_CSR, n, end_offset, max_text_len, d_text_prefix, d_entries, d_spans,
                     span_cap, total, stream);
}
int mrx_kw_leftmost_strided_dev(const mrx_kw* k, int64_t count, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                                int32_t len, int64_t n, int64_t* d_text_prefix, int32_t* d_entries, int32_t* d_spans,
                                int64_t span_cap, int64_t* total, void* stream) {
  return kw_leftmost(k, count, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1, -1, d_text_prefix, d_entries, d_spans,
                     span_cap, total, stream);
}

int mrx_kw_sub_dev(const mrx_kw* k, const uint8_t* d_repl_data, const int64_t* d_repl_offsets, int64_t r, int64_t count,
                   const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_out_offsets, uint8_t* d_out_data,
                   int64_t out_cap, int32_t* d_nsub, int64_t* d_totals, int64_t* totals, void* stream) {
  return kw_sub(k, csr(d_data, d_offsets), BATCH_CSR, n, -1, -1,
                SubArgs{d_repl_data, d_repl_offsets, r, count, d_out_offsets, d_out_data, out_cap, d_nsub, d_totals, totals, stream});
}
int mrx_kw_sub_known_dev(const mrx_kw* k, const uint8_t* d_repl_data, const int64_t* d_repl_offsets, int64_t r, int64_t count,
                         const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len,
                         int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int32_t* d_nsub, int64_t* d_totals,
                         int64_t* totals, void* stream) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return kw_sub(k, csr(d_data, d_offsets), BATCH_CSR, n, end_offset, max_text_len,
                SubArgs{d_repl_data, d_repl_offsets, r, count, d_out_offsets, d_out_data, out_cap, d_nsub, d_totals, totals, stream});
}
int mrx_kw_sub_strided_dev(const mrx_kw* k, const uint8_t* d_repl_data, const int64_t* d_repl_offsets, int64_t r, int64_t count,
                           const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                           int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int32_t* d_nsub, int64_t* d_totals,
                           int64_t* totals, void* stream) {
  return kw_sub(k, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1, -1,
                SubArgs{d_repl_data, d_repl_offsets, r, count, d_out_offsets, d_out_data, out_cap, d_nsub, d_totals, totals, stream});
}

// host buffers: argument errors before any device work, as the _dev entry points
int mrx_kw_leftmost_batch(const mrx_kw* k, int64_t count, const uint8_t* data, const int64_t* offsets, int64_t n,
                          int64_t* text_prefix, int32_t* entries, int32_t* spans, int64_t span_cap, int64_t* total) {
  if (!k || n < 0 || !offsets || !text_prefix || (span_cap > 0 && (!entries || !spans)))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (span_cap < 0 || count < 0) return internal_fail(MRX_E_ARGUMENT, "span_cap and count must be >= 0");
  DevBatch b;
  DevBuf<int64_t> pre;
  DevBuf<int32_t> en;
  DevBuf<uint64_t> sp;   // (8-byte aligned whatever the allocator)
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = pre.alloc((size_t)n + 1)) return rc;
  if (int rc = en.alloc((size_t)span_cap)) return rc;
  if (int rc = sp.alloc((size_t)span_cap)) return rc;
  int64_t tot = 0;
  const int rc = mrx_kw_leftmost_known_dev(k, count, b.data, b.offsets, n, b.nbytes, b.longest, pre.p, en.p, (int32_t*)sp.p,
                                           span_cap, &tot, nullptr);
  if (total) *total = tot;
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  MRX_HIP_TRY(hipMemcpy(text_prefix, pre.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot > 0) {
    MRX_HIP_TRY(hipMemcpy(entries, en.p, sizeof(int32_t) * (size_t)tot, hipMemcpyDeviceToHost));
    MRX_HIP_TRY(hipMemcpy(spans, sp.p, sizeof(int32_t) * 2 * (size_t)tot, hipMemcpyDeviceToHost));
  }
  return rc;
}
int mrx_kw_sub_batch(const mrx_kw* k, const uint8_t* repl_data, const int64_t* repl_offsets, int64_t r, int64_t count,
                     const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data,
                     int64_t out_cap, int32_t* nsub, int64_t* totals) {
  if (!k || n < 0 || !offsets || !out_offsets || (out_cap > 0 && !out_data)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (out_cap < 0 || count < 0 || r < 0) return internal_fail(MRX_E_ARGUMENT, "out_cap, count and r must be >= 0");
  if (r > 0 && (!repl_data || !repl_offsets)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (r != 1 && r != k->m) return internal_fail(MRX_E_ARGUMENT, "r must be 1 or the number of entries, " + std::to_string(k->m));
  DevBatch b, rp;
  DevBuf<int64_t> oo;
  DevBuf<uint8_t> od;
  DevBuf<int32_t> ns;
  if (int rc = b.measure(offsets, n)) return rc;
  if (int rc = rp.measure(repl_offsets, r)) return rc;
  if (b.nbytes < 0 || rp.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = rp.upload(repl_data, repl_offsets, r)) return rc;
  if (int rc = oo.alloc((size_t)n + 1)) return rc;
  if (int rc = od.alloc((size_t)out_cap)) return rc;
  if (int rc = ns.alloc((size_t)n)) return rc;
  int64_t tot[3] = {0, 0, 0};
  const int rc = mrx_kw_sub_known_dev(k, rp.data, rp.offsets, r, count, b.data, b.offsets, n, b.nbytes, b.longest, oo.p, od.p,
                                      out_cap, ns.p, nullptr, tot, nullptr);
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  if (totals) totals[0] = tot[0], totals[1] = tot[1], totals[2] = tot[2];
  MRX_HIP_TRY(hipMemcpy(out_offsets, oo.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost));
  if (nsub && n > 0) MRX_HIP_TRY(hipMemcpy(nsub, ns.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot[0] > 0) MRX_HIP_TRY(hipMemcpy(out_data, od.p, (size_t)tot[0], hipMemcpyDeviceToHost));
  return rc;
}

int mrx_debug_kw_host_leftmost(const uint8_t* entry_data, const int64_t* entry_offsets, int64_t m, uint32_t flags, int64_t count,
                               const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* text_prefix, int32_t* entries,
                               int32_t* spans, int64_t span_cap, int64_t* total) {
  if (count < 0 || span_cap < 0) return internal_fail(MRX_E_ARGUMENT, "count and span_cap must be >= 0");
  if (int rc = host_check_texts(data, offsets, n)) return rc;
  if (!text_prefix || (span_cap > 0 && (!entries || !spans))) return internal_fail(MRX_E_ARGUMENT, "null argument");
  KwAutomaton A;
  if (int rc = host_reversed(entry_data, entry_offsets, m, flags, &A)) return rc;
  HostPlaced t;
  t.place(data, offsets, n);
  const int64_t pinned = kw_pinned_piece();
  const int64_t P = pinned > 0 ? pinned : kw_piece_rule(A.lmax, t.rel[(size_t)n]);
  KwSubHostResult res;
  kw_sub_host(A, P, count, t.p, t.rel.data(), n, false, KwRepl{nullptr, nullptr, 1}, nullptr, 0, span_cap, &res);
  for (int64_t i = 0; i <= n; ++i) text_prefix[i] = res.kb[(size_t)i];
  const int64_t tot = res.kb[(size_t)n];
  if (total) *total = tot;
  if (tot > span_cap) return internal_fail(MRX_E_CAPACITY, "span buffer too small: need " + std::to_string(tot));
  for (int64_t g = 0; g < tot; ++g) {
    entries[g] = res.entries[(size_t)g];
    spans[2 * g] = (int32_t)(uint32_t)res.spans[(size_t)g];
    spans[2 * g + 1] = (int32_t)(uint32_t)(res.spans[(size_t)g] >> 32);
  }
  return MRX_OK;
}

int mrx_debug_kw_host_sub(const uint8_t* entry_data, const int64_t* entry_offsets, int64_t m, uint32_t flags,
                          const uint8_t* repl_data, const int64_t* repl_offsets, int64_t r, int64_t count, const uint8_t* data,
                          const int64_t* offsets, int64_t n, int64_t* out_offsets, uint8_t* out_data, int64_t out_cap,
                          int32_t* nsub, int64_t* totals) {
  if (count < 0 || r < 0 || out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "count, r and out_cap must be >= 0");
  if (int rc = host_check_texts(data, offsets, n)) return rc;
  if (!out_offsets || (out_cap > 0 && !out_data)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (r > 0) {
    if (!repl_offsets) return internal_fail(MRX_E_ARGUMENT, "null argument");
    if (int rc = host_check_texts(repl_data, repl_offsets, r)) return rc;
  }
  KwAutomaton A;
  if (int rc = host_reversed(entry_data, entry_offsets, m, flags, &A)) return rc;
  if (r != 1 && r != m) return internal_fail(MRX_E_ARGUMENT, "r must be 1 or the number of entries, " + std::to_string(m));
  HostPlaced t, rp;
  t.place(data, offsets, n);
  rp.place(repl_data, repl_offsets, r);
  const int64_t pinned = kw_pinned_piece();
  const int64_t P = pinned > 0 ? pinned : kw_piece_rule(A.lmax, t.rel[(size_t)n]);
  KwSubHostResult res;
  kw_sub_host(A, P, count, t.p, t.rel.data(), n, true, KwRepl{rp.p, rp.rel.data(), r}, out_data, out_cap, 0, &res);
  for (int64_t i = 0; i <= n; ++i) out_offsets[i] = res.out_off[(size_t)i];
  for (int64_t i = 0; i < n && nsub; ++i) nsub[i] = (int32_t)(res.kb[(size_t)i + 1] - res.kb[(size_t)i]);
  if (totals) totals[0] = res.bytes, totals[1] = res.longest, totals[2] = res.kb[(size_t)n];
  if (res.bytes > out_cap) return internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(res.bytes));
  return MRX_OK;
}

}  // extern "C"
