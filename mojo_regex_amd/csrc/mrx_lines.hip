// Lines (include/mrx.h, "lines"): a batch's texts cut at one separator byte into a new packed CSR batch on the device.
// The block walk, the pieces and the order of the passes are in mrx_lines_bits.hpp; here are the kernels, the launches
// and the entry points.
//
//   k_lines_pieces        (CSR) ceil(len / P) per text; the existing exclusive scan makes the first piece of every text
//   k_lines_count         a wavefront per piece: separators, kept bytes, bytes behind the last separator
//   exclusive_scan        of the separators and of the kept bytes over the pieces
//   k_lines_text          per text: tail, lines, output bytes; d_totals[3], d_out_offsets[0]
//   exclusive_scan        of the lines into d_line_prefix (sum -> d_totals[0]) and of the bytes (sum -> d_totals[1])
//   k_lines_emit          a wavefront per piece: offsets, owners and the compacted bytes
//   k_lines_longest(_end) the longest line from the finished offsets -> d_totals[2]
// The text-major pieces, the wavefront's way from a piece to its text and the LDS stage through which the emit kernel's
// kept bytes leave as aligned 16-byte blocks are in mrx_pieces.hpp, shared with translate.
// No atomics, no inline assembly, and no wavefront waits for another one: every scan is a launch of its own.
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
#include "mrx_lines_bits.hpp"
#include "mrx_pieces.hpp"

namespace mrx {
namespace {

constexpr int kLinesBlock = 256, kLinesWaves = kLinesBlock / 64;
constexpr unsigned kLinesMaxGrid = 2048;    // 8 workgroups per CU; the kernels stride over what is left
constexpr int kLinesParts = 1024;           // partial maxima of the longest line
constexpr int64_t kLinesPieceMax = 1 << 20;

std::atomic<int64_t> g_lines_piece{0};
std::atomic<int64_t> g_lines_syncs{0};

int64_t lines_piece() {
  const int64_t pinned = g_lines_piece.load();
  return pinned > 0 ? pinned : kLinesPiece;
}

// what the passes leave for each other (scratch)
struct LinesWork {
  int64_t* nsep;        // [npieces]
  int64_t* kept;        // [npieces]
  int64_t* after;       // [npieces]
  int64_t* sep_scan;    // [npieces + 1]
  int64_t* kept_scan;   // [npieces + 1]
  int64_t* tlines;      // [n]
  int64_t* tbytes;      // [n]
  int64_t* tails;       // [n]
  int64_t* tbase;       // [n + 1] every text's first output byte
};
__global__ __launch_bounds__(kLinesBlock) void k_lines_count(const TextBatch B, int64_t n, const LinesPieces pc, uint32_t sep,
                                                             uint32_t flags, const LinesWork W) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int64_t piece = (int64_t)blockIdx.x * kLinesWaves + wave; piece < pc.npieces; piece += (int64_t)gridDim.x * kLinesWaves) {
    const LinesJob job = lines_job(B, n, pc, piece);
    int ns = 0, kp = 0, last = -1;
    for (int64_t q = job.p0 + 16 * lane; q < job.pend; q += kLinesRound) {
      const LinesBlock b = lines_block(job.tp, job.L, q, job.L, sep, flags);
      ns += lines_popc(b.sep);
      kp += lines_popc(b.keep);
      if (b.sep) last = (int)(q - job.p0) + 31 - __clz((int)b.sep);
    }
    ns = wave_sum(ns);
    kp = wave_sum(kp);
    last = wave_max(last);
    if (lane == 0) {
      W.nsep[piece] = ns;
      W.kept[piece] = kp;
      W.after[piece] = (job.pend - job.p0) - (last + 1);
    }
  }
}

__global__ __launch_bounds__(256) void k_lines_text(const TextBatch B, int64_t n, const LinesPieces pc, uint32_t flags,
                                                    const LinesWork W, int64_t* __restrict__ out_offsets,
                                                    int64_t* __restrict__ totals) {
  const bool drop_tail = (flags & MRX_LINES_DROP_PARTIAL) != 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t L;
    (void)lines_text(B, i, &L);
    int64_t a = pc.first ? pc.first[i] : i * pc.per_text, b = pc.first ? pc.first[i + 1] : a + pc.per_text;
    a = a < pc.npieces ? a : pc.npieces;   // (only offsets that break the contract put a text's pieces behind the scans)
    b = b < pc.npieces ? b : pc.npieces;
    const int64_t tail = L > 0 && b > a ? lines_tail(W.sep_scan, W.after, a, b, L, pc.P) : 0;
    W.tails[i] = tail;
    W.tlines[i] = (W.sep_scan[b] - W.sep_scan[a]) + (!drop_tail && tail > 0 ? 1 : 0);
    W.tbytes[i] = (W.kept_scan[b] - W.kept_scan[a]) - (drop_tail ? tail : 0);
    if (i == n - 1) totals[3] = tail;
    if (i == 0) out_offsets[0] = 0;
  }
}

// what the emit kernel reads and writes beside the batch
struct LinesOut {
  const int64_t* line_prefix;   // [n + 1]
  const int64_t* totals;        // {lines, bytes}: written by the scans in front
  int64_t* owner;
  int64_t* out_offsets;
  int64_t piece_cap;
  uint8_t* out;
  int64_t out_cap;
};

__shared__ g_u64x2 s_lines_stage[kLinesWaves][kLinesStage / 16];

__global__ __launch_bounds__(kLinesBlock) void k_lines_emit(const TextBatch B, int64_t n, const LinesPieces pc, uint32_t sep,
                                                            uint32_t flags, const LinesWork W, const LinesOut O) {
  const int64_t lines = O.totals[0], bytes = O.totals[1];
  if (lines > O.piece_cap) return;
  const bool move = bytes > 0 && bytes <= O.out_cap;
  const bool drop_tail = (flags & MRX_LINES_DROP_PARTIAL) != 0;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  g_u64x2* stage16 = s_lines_stage[wave];
  for (int64_t piece = (int64_t)blockIdx.x * kLinesWaves + wave; piece < pc.npieces; piece += (int64_t)gridDim.x * kLinesWaves) {
    const LinesJob job = lines_job(B, n, pc, piece);
    const bool has = job.pend > job.p0;
    int64_t line = 0, pos = 0, limit = 0;
    if (has) {
      line = O.line_prefix[job.text] + (W.sep_scan[piece] - W.sep_scan[job.a]);
      pos = W.tbase[job.text] + (W.kept_scan[piece] - W.kept_scan[job.a]);
      limit = job.L - (drop_tail ? W.tails[job.text] : 0);
    }
    LinesStage st = lines_stage_open(has && move, O.out, pos);
    for (int64_t q0 = job.p0; q0 < job.pend; q0 += kLinesRound) {   // (a short text's piece ends after its first round)
      const int64_t q = q0 + 16 * lane;
      const LinesBlock b = q < job.pend ? lines_block(job.tp, job.L, q, limit, sep, flags) : lines_no_block();
      const uint32_t mine = (uint32_t)lines_popc(b.keep) | ((uint32_t)lines_popc(b.ends) << 16);
      uint32_t inc = mine;   // kept bytes below, line ends above: a round has at most 1024 of either
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
      }
      const uint32_t all = __shfl(inc, 63), before = inc - mine;
      const int K = (int)(all & 0xffffu), kept_before = (int)(before & 0xffffu);
      int64_t j = line + (before >> 16);
      for (uint32_t m = b.ends; m; m &= m - 1) {
        O.out_offsets[j + 1] = pos + kept_before + lines_kept_through(b, __ffs((int)m) - 1);
        O.owner[j++] = job.text;
      }
      line += all >> 16;
      pos += K;
      if (move) lines_stage_round(st, stage16, lane, b.bytes, b.keep, kept_before, K);
    }
    if (move) lines_stage_close(st, stage16, lane);
  }
}

__global__ __launch_bounds__(256) void k_lines_longest(const int64_t* __restrict__ out_offsets, const int64_t* __restrict__ totals,
                                                       int64_t piece_cap, int64_t* __restrict__ part) {
  __shared__ int64_t wmax[4];
  const int64_t lines = totals[0] <= piece_cap ? totals[0] : 0;
  int64_t m = 0;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < lines; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t len = out_offsets[j + 1] - out_offsets[j];
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
__global__ __launch_bounds__(64) void k_lines_longest_end(const int64_t* __restrict__ part, int nparts, int64_t* __restrict__ totals) {
  int64_t m = 0;
  for (int k = (int)threadIdx.x; k < nparts; k += 64) m = part[k] > m ? part[k] : m;
  for (int off = 32; off > 0; off >>= 1) {
    const int64_t y = __shfl_xor(m, off);
    m = y > m ? y : m;
  }
  if (threadIdx.x == 0) totals[2] = m;
}

// argument errors: nothing has touched the device when one of them returns.  The options, which the host-buffer forms
// share ...
int lines_check_options(uint32_t flags, uint8_t sep, int64_t n, int64_t piece_cap, int64_t out_cap) {
  if (flags & ~kLinesFlags) return internal_fail(MRX_E_ARGUMENT, "unknown flag bits");
  if ((flags & MRX_LINES_CRLF) && (sep != '\n' || (flags & MRX_LINES_KEEPENDS)))
    return internal_fail(MRX_E_ARGUMENT, "MRX_LINES_CRLF needs the separator '\\n' and no MRX_LINES_KEEPENDS");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (piece_cap < 0 || out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "piece_cap and out_cap must be >= 0");
  return MRX_OK;
}
// ... and the batch and the pointers of a device call
int lines_check(uint32_t flags, uint8_t sep, const TextBatch& b, BatchForm form, int64_t n, const int64_t* d_line_prefix,
                int64_t piece_cap, const PackedDest& o) {
  if (int rc = lines_check_options(flags, sep, n, piece_cap, o.out_cap)) return rc;
  if (int rc = check_batch(b, form)) return rc;
  if (!d_line_prefix || !o.d_out_offsets || !o.d_totals || (piece_cap > 0 && !o.d_rows) || (o.out_cap > 0 && !o.d_out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  return MRX_OK;
}

// the launches on a checked batch of n >= 1 texts whose pieces and scratch are set up
int lines_enqueue(uint32_t flags, uint8_t sep, const TextBatch& b, int64_t n, const LinesPieces& pc, const LinesWork& W,
                  int64_t* dummy, int64_t* part, int64_t* d_line_prefix, int64_t piece_cap, const PackedDest& o);

// known_total: a CSR batch's byte count where the caller has it (an upper bound is fine), < 0: read back
int lines_run(uint32_t flags, uint8_t sep, const TextBatch& b, BatchForm form, int64_t n, int64_t known_total,
              int64_t* d_line_prefix, int64_t piece_cap, const PackedDest& o) {
  if (int rc = lines_check(flags, sep, b, form, n, d_line_prefix, piece_cap, o)) return rc;
  hipStream_t hs = (hipStream_t)o.stream;
  if (n == 0) {
    MRX_HIP_TRY(hipMemsetAsync(d_line_prefix, 0, sizeof(int64_t), hs));
    set_last_kernel("k_lines_emit");
    return packed_empty(o, 4);
  }
  ScratchScope scope_(o.stream);
  LinesPieces pc{lines_piece(), 0, nullptr, 0};
  int64_t* dummy = (int64_t*)scratch_get(sizeof(int64_t) * 2, o.stream);   // the sums of the scans that nobody reads
  if (!dummy) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  if (int rc = lines_pieces_setup(b, n, known_total, dummy, g_lines_syncs, o.stream, &pc)) return rc;
  LinesWork W;
  const size_t np = (size_t)pc.npieces, i64 = sizeof(int64_t);
  W.nsep = (int64_t*)scratch_get(i64 * np, o.stream);
  W.kept = (int64_t*)scratch_get(i64 * np, o.stream);
  W.after = (int64_t*)scratch_get(i64 * np, o.stream);
  W.sep_scan = (int64_t*)scratch_get(i64 * (np + 1), o.stream);
  W.kept_scan = (int64_t*)scratch_get(i64 * (np + 1), o.stream);
  W.tlines = (int64_t*)scratch_get(i64 * (size_t)n, o.stream);
  W.tbytes = (int64_t*)scratch_get(i64 * (size_t)n, o.stream);
  W.tails = (int64_t*)scratch_get(i64 * (size_t)n, o.stream);
  W.tbase = (int64_t*)scratch_get(i64 * (size_t)(n + 1), o.stream);
  int64_t* part = (int64_t*)scratch_get(i64 * kLinesParts, o.stream);
  if (!W.nsep || !W.kept || !W.after || !W.sep_scan || !W.kept_scan || !W.tlines || !W.tbytes || !W.tails || !W.tbase || !part)
    return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  void* timer = scan_timer_begin(o.stream);   // (mrx_timing_scan_ms: the kernels apart from the call)
  const int rc = lines_enqueue(flags, sep, b, n, pc, W, dummy, part, d_line_prefix, piece_cap, o);
  scan_timer_end(timer);
  if (rc) return rc;
  set_last_kernel("k_lines_emit");
  if (o.totals) ++g_lines_syncs;
  return packed_verdict(o, piece_cap, nullptr, 4);
}

int lines_enqueue(uint32_t flags, uint8_t sep, const TextBatch& b, int64_t n, const LinesPieces& pc, const LinesWork& W,
                  int64_t* dummy, int64_t* part, int64_t* d_line_prefix, int64_t piece_cap, const PackedDest& o) {
  hipStream_t hs = (hipStream_t)o.stream;
  const unsigned grid = grid_for(pc.npieces, kLinesWaves, kLinesMaxGrid), tgrid = grid_for(n, 256, 4096);
  hipLaunchKernelGGL(k_lines_count, dim3(grid), dim3(kLinesBlock), 0, hs, b, n, pc, (uint32_t)sep, flags, W);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(W.nsep, pc.npieces, W.sep_scan, dummy, o.stream)) return rc;
  if (int rc = exclusive_scan(W.kept, pc.npieces, W.kept_scan, dummy + 1, o.stream)) return rc;
  hipLaunchKernelGGL(k_lines_text, dim3(tgrid), dim3(256), 0, hs, b, n, pc, flags, W, o.d_out_offsets, o.d_totals);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(W.tlines, n, d_line_prefix, o.d_totals, o.stream)) return rc;
  if (int rc = exclusive_scan(W.tbytes, n, W.tbase, o.d_totals + 1, o.stream)) return rc;
  if (piece_cap > 0) {   // (no line fits a capacity of 0)
    const LinesOut O{d_line_prefix, o.d_totals, o.d_rows, o.d_out_offsets, piece_cap, o.d_out_data, o.out_cap};
    hipLaunchKernelGGL(k_lines_emit, dim3(grid), dim3(kLinesBlock), 0, hs, b, n, pc, (uint32_t)sep, flags, W, O);
    MRX_HIP_TRY(hipGetLastError());
  }
  const unsigned lgrid = grid_for(piece_cap, 256 * 8, kLinesParts);
  hipLaunchKernelGGL(k_lines_longest, dim3(lgrid), dim3(256), 0, hs, o.d_out_offsets, o.d_totals, piece_cap, part);
  hipLaunchKernelGGL(k_lines_longest_end, dim3(1), dim3(64), 0, hs, part, (int)lgrid, o.d_totals);
  MRX_HIP_TRY(hipGetLastError());
  return MRX_OK;
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_lines_dev(uint32_t flags, uint8_t sep, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                  int64_t* d_line_prefix, int64_t* d_owner, int64_t* d_out_offsets, int64_t piece_cap, uint8_t* d_out_data,
                  int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return lines_run(flags, sep, csr(d_data, d_offsets), BATCH_CSR, n, -1, d_line_prefix, piece_cap,
                   PackedDest{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream});
}
int mrx_lines_known_dev(uint32_t flags, uint8_t sep, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                        int64_t end_offset, int64_t max_text_len, int64_t* d_line_prefix, int64_t* d_owner,
                        int64_t* d_out_offsets, int64_t piece_cap, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                        int64_t* totals, void* stream) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return lines_run(flags, sep, csr(d_data, d_offsets), BATCH_CSR, n, end_offset, d_line_prefix, piece_cap,
                   PackedDest{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream});
}
int mrx_lines_strided_dev(uint32_t flags, uint8_t sep, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                          int32_t len, int64_t n, int64_t* d_line_prefix, int64_t* d_owner, int64_t* d_out_offsets,
                          int64_t piece_cap, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                          void* stream) {
  return lines_run(flags, sep, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1, d_line_prefix, piece_cap,
                   PackedDest{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream});
}

// host buffers: argument errors before any device work, as the _dev entry points
int mrx_lines_batch(uint32_t flags, uint8_t sep, const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* line_prefix,
                    int64_t* owner, int64_t* out_offsets, int64_t piece_cap, uint8_t* out_data, int64_t out_cap,
                    int64_t* totals) {
  const HostOut o{owner, out_offsets, out_data, totals};
  if (int rc = host_out_check(n, piece_cap, out_cap, offsets, o)) return rc;
  if (!line_prefix) return internal_fail(MRX_E_ARGUMENT, "null argument");
  DevBatch b; DevBuf<int64_t> pre, ow, oo, dt; DevBuf<uint8_t> od;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = lines_check_options(flags, sep, n, piece_cap, out_cap)) return rc;
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = pre.alloc((size_t)n + 1)) return rc;
  if (int rc = ow.alloc((size_t)piece_cap)) return rc;
  if (int rc = oo.alloc((size_t)piece_cap + 1)) return rc;
  if (int rc = dt.alloc(4)) return rc;
  if (int rc = od.alloc((size_t)out_cap)) return rc;
  int64_t tot[4] = {0, 0, 0, 0};
  const int rc = mrx_lines_known_dev(flags, sep, b.data, b.offsets, n, b.nbytes, b.longest, pre.p, ow.p, oo.p, piece_cap, od.p, out_cap, dt.p, tot, nullptr);
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  if (totals) memcpy(totals, tot, sizeof tot);
  MRX_HIP_TRY(hipMemcpy(line_prefix, pre.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost));
  if (tot[0] > piece_cap) return rc;
  if (tot[0] > 0) MRX_HIP_TRY(hipMemcpy(owner, ow.p, sizeof(int64_t) * (size_t)tot[0], hipMemcpyDeviceToHost));
  MRX_HIP_TRY(hipMemcpy(out_offsets, oo.p, sizeof(int64_t) * (size_t)(tot[0] + 1), hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot[1] > 0) MRX_HIP_TRY(hipMemcpy(out_data, od.p, (size_t)tot[1], hipMemcpyDeviceToHost));
  return rc;
}

int64_t mrx_debug_lines_piece(int64_t bytes) {
  if (bytes >= 0) {
    int64_t P = (bytes + kLinesRound - 1) / kLinesRound * kLinesRound;
    g_lines_piece.store(P > kLinesPieceMax ? kLinesPieceMax : P);
  }
  return lines_piece();
}
int64_t mrx_debug_lines_syncs(void) { return g_lines_syncs.load(); }

int mrx_debug_lines_host(uint32_t flags, uint8_t sep, const uint8_t* data, const int64_t* offsets, int64_t n,
                         int64_t* line_prefix, int64_t* owner, int64_t* out_offsets, int64_t piece_cap, uint8_t* out_data,
                         int64_t out_cap, int64_t* totals) {
  if (int rc = host_out_check(n, piece_cap, out_cap, offsets, HostOut{owner, out_offsets, out_data, totals})) return rc;
  if (!line_prefix) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = lines_check_options(flags, sep, n, piece_cap, out_cap)) return rc;
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  const int64_t bytes = n > 0 ? offsets[n] - offsets[0] : 0;
  if (bytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  // the texts at their own alignment inside a buffer that owns the aligned words around them
  const size_t skew = n > 0 && data ? (size_t)((uintptr_t)(data + offsets[0]) & 15) : 0;
  std::vector<g_u64x2> room((size_t)bytes / 16 + 3);
  uint8_t* copy = (uint8_t*)room.data() + skew;
  if (bytes > 0) memcpy(copy, data + offsets[0], (size_t)bytes);
  std::vector<int64_t> rel((size_t)n + 1, 0);
  for (int64_t i = 0; i <= n && n > 0; ++i) rel[(size_t)i] = offsets[i] - offsets[0];
  int64_t tot[4] = {0, 0, 0, 0};
  lines_host(copy, rel.data(), n, lines_piece(), sep, flags, LinesHostOut{line_prefix, owner, out_offsets, piece_cap, out_data, out_cap, tot});
  if (totals) memcpy(totals, tot, sizeof tot);
  if (tot[0] > piece_cap) return internal_fail(MRX_E_CAPACITY, "piece buffers too small: need " + std::to_string(tot[0]));
  if (tot[1] > out_cap) return internal_fail(MRX_E_CAPACITY, "output buffer too small: need " + std::to_string(tot[1]));
  return MRX_OK;
}

}  // extern "C"
