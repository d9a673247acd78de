// Extract (include/mrx.h, "extract"): the bytes under spans -- findall's matches, split's pieces, one group of every
// captures_all row, a set's hits -- gathered into a new packed CSR batch on the device, in row order.
//
// Route.  The primitive takes a CSR of rows over the texts and the rows' (start, end) pairs:
//   k_extract_sizes   a lane per row: its text by bisection of the row CSR, the clamped range, then the owner, the
//                     piece's length and its absolute source position (scratch)
//   exclusive_scan    of the lengths over the host-known piece_cap, straight into d_out_offsets; sum -> d_totals[1]
//   k_extract_gather  the bytes
// mrx_extract_* puts findall in front (member_findall into scratch, no host total).  Nothing looks at the device in
// between: the kernels read pieces and bytes from d_totals and write no byte when either capacity is short.  With a
// host `totals` the call reads d_totals back once, at the end.
//
// The gather is the block walk that filter's block form has too (gather_blocks, mrx_gather_bits.hpp) with a fill of its
// own.  A piece's source is its position from the sizes kernel, not a text index: a short match shares
// its block with others (a lone [a-z]+\d+ token is about 6 bytes; the headline batch averages 26 bytes a piece, its
// full-text matches included), each at an address the one before does not predict, so the lane walks the
// pieces of its block and steps over runs of empty ones by galloping (an empty piece repeats its offset: the last
// piece at or below a position is never empty).  One form only: work is balanced by output bytes, so a multi-megabyte
// split piece is spread over every wavefront and a run of short matches fills blocks lane by lane.  Filter's text
// form (16 lanes a row) would leave 15 lanes idle on a piece of a few bytes.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_gather_bits.hpp"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"

namespace mrx {
namespace {

constexpr int kExtractBlock = 256;
constexpr unsigned kExtractMaxGrid = 2048;   // 8 workgroups per CU; the kernels stride over what is left

std::atomic<int> g_extract_grid{0};   // mrx_debug_extract_grid(): workgroups of the gather at most (0 = no cap of its own)

// where the pieces go and the rows: the arguments behind the batch of mrx_gather_spans_dev
struct SpanArgs : PackedDest {   // d_rows: d_owner
  const int64_t* d_prefix;
  const int32_t* d_spans;
  int32_t row_pairs, pair;
  int64_t piece_cap;
};

// what the sizes kernel and the scan wrote and the gather reads
struct ExtractOut {
  const uint8_t* data;       // the batch's bytes
  const int64_t* src;        // [pieces] absolute position of each piece's first byte in `data`
  const int64_t* out_off;    // [pieces + 1] CSR of the output
  const int64_t* totals;     // {pieces, bytes}
  int64_t piece_cap;
  uint8_t* out;
  int64_t out_cap;
};

// Rows that do not all fit get no owner and length 0 (the spans are not read: bytes is then 0, a lower bound).
__global__ __launch_bounds__(kExtractBlock) void k_extract_sizes(const TextBatch B, int64_t n,
                                                                 const int64_t* __restrict__ prefix,
                                                                 const int32_t* __restrict__ spans, int row_pairs, int pair,
                                                                 int64_t piece_cap, int64_t* __restrict__ owner,
                                                                 int64_t* __restrict__ plen, int64_t* __restrict__ src,
                                                                 int64_t* __restrict__ totals) {
  const int64_t pieces = prefix[n];
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (first == 0) totals[0] = pieces;
  const int64_t rows = pieces <= piece_cap ? pieces : 0;
  for (int64_t r = first; r < piece_cap; r += (int64_t)gridDim.x * blockDim.x) {
    if (r >= rows) {
      plen[r] = 0;
      continue;
    }
    const int64_t i = gather_last_le(prefix, 0, n, r);   // prefix[i] <= r < prefix[i + 1]: texts without rows are passed
    int32_t L;
    const uint8_t* tp = B.text(i, &L);
    const int2 se = *(const int2*)(spans + 2 * (r * row_pairs + pair));
    const int32_t s = se.x < 0 ? 0 : se.x < L ? se.x : L;
    const int32_t e = se.y < s ? s : se.y < L ? se.y : L;
    owner[r] = i;
    plen[r] = e - s;
    src[r] = (int64_t)(tp - B.data) + s;
  }
}

__global__ __launch_bounds__(kExtractBlock) void k_extract_gather(const ExtractOut O) {
  const int64_t pieces = O.totals[0], bytes = O.totals[1];
  if (pieces > O.piece_cap || bytes <= 0 || bytes > O.out_cap) return;
  gather_blocks<kExtractBlock>(O.out, bytes, O.out_off, pieces, [&](int64_t r, int64_t hi, int64_t p0, int64_t pos, int64_t endp) {
    g_u128 acc = 0;
    while (true) {   // piece r holds byte pos
      const int64_t s = O.out_off[r], e = O.out_off[r + 1];
      const int take = (int)((e < endp ? e : endp) - pos);
      acc = gather_place(acc, O.data + O.src[r] + (pos - s), take, (int)(pos - p0));
      pos += take;
      if (pos >= endp) break;
      r = gather_gallop(O.out_off, r + 1, hi + 1, pos);   // the next piece with a byte: empty ones are stepped over
    }
    return acc;
  });
}

// argument errors: nothing has touched the device when one of them returns.  own_spans: the spans are the call's own
// (mrx_extract_*: findall's, in scratch)
int gather_check(const TextBatch& b, BatchForm form, int64_t n, const SpanArgs& a, bool own_spans) {
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (a.piece_cap < 0 || a.out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "piece_cap and out_cap must be >= 0");
  if (a.row_pairs < 1) return internal_fail(MRX_E_ARGUMENT, "row_pairs must be >= 1");
  if (a.pair < 0 || a.pair >= a.row_pairs) return internal_fail(MRX_E_ARGUMENT, "pair must be in [0, row_pairs)");
  if ((uintptr_t)a.d_spans & 7) return internal_fail(MRX_E_ARGUMENT, "d_spans must be 8-byte aligned");
  if (int rc = check_batch(b, form)) return rc;
  if (!a.d_prefix || !a.d_out_offsets || !a.d_totals || (a.piece_cap > 0 && (!a.d_rows || (!own_spans && !a.d_spans))) ||
      (a.out_cap > 0 && !a.d_out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  return MRX_OK;
}

int gather_empty(const SpanArgs& a) {   // n == 0
  if (int rc = packed_empty(a)) return rc;
  set_last_kernel("k_extract_gather");
  return MRX_OK;
}

// the three device steps on a checked batch with n > 0, inside the caller's ScratchScope; d_prefix[n] and the spans
// may still be on their way on a.stream
int gather_enqueue(const TextBatch& b, int64_t n, const SpanArgs& a) {
  hipStream_t hs = (hipStream_t)a.stream;
  const size_t cap = (size_t)(a.piece_cap > 0 ? a.piece_cap : 1);
  int64_t* plen = (int64_t*)scratch_get(sizeof(int64_t) * cap, a.stream);
  int64_t* src = (int64_t*)scratch_get(sizeof(int64_t) * cap, a.stream);
  if (!plen || !src) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  const dim3 blk(kExtractBlock);
  hipLaunchKernelGGL(k_extract_sizes, dim3(grid_for(a.piece_cap, kExtractBlock, kExtractMaxGrid)), blk, 0, hs, b, n, a.d_prefix,
                     a.d_spans, (int)a.row_pairs, (int)a.pair, a.piece_cap, a.d_rows, plen, src, a.d_totals);
  MRX_HIP_TRY(hipGetLastError());
  if (int rc = exclusive_scan(plen, a.piece_cap, a.d_out_offsets, a.d_totals + 1, a.stream)) return rc;
  if (a.out_cap > 0 && a.piece_cap > 0) {   // (nothing fits a capacity of 0, and no empty output has a byte to move)
    const ExtractOut O{b.data, src, a.d_out_offsets, a.d_totals, a.piece_cap, a.d_out_data, a.out_cap};
    // a wavefront per 64 blocks = 1 KiB of output at least
    const unsigned grid = grid_for(a.out_cap / 16 + 2, kExtractBlock, kExtractMaxGrid, g_extract_grid.load(std::memory_order_relaxed));
    hipLaunchKernelGGL(k_extract_gather, dim3(grid), blk, 0, hs, O);
    MRX_HIP_TRY(hipGetLastError());
  }
  set_last_kernel("k_extract_gather");
  return packed_verdict(a, a.piece_cap);
}

int gather_run(const TextBatch& b, BatchForm form, int64_t n, const SpanArgs& a) {
  if (int rc = gather_check(b, form, n, a, false)) return rc;
  if (n == 0) return gather_empty(a);
  ScratchScope scope_(a.stream);
  return gather_enqueue(b, n, a);
}

// findall's spans into scratch, then the primitive.  Argument errors, then findall's refusals (its own text), before
// anything is enqueued.
int extract_run(const mrx_handle* h, const TextBatch& b, BatchForm form, int64_t n, int64_t known_total, int64_t known_max,
                int64_t* d_piece_prefix, SpanArgs a) {
  if (!h) return internal_fail(MRX_E_ARGUMENT, "null handle");
  a.d_prefix = d_piece_prefix;
  if (int rc = gather_check(b, form, n, a, true)) return rc;
  const std::string refused = handle_refusal(h);
  if (!refused.empty()) return internal_fail(MRX_E_UNSUPPORTED, refused);
  if (n == 0) {
    MRX_HIP_TRY(hipMemsetAsync(d_piece_prefix, 0, sizeof(int64_t), (hipStream_t)a.stream));
    return gather_empty(a);
  }
  ScratchScope scope_(a.stream);
  // a result that fits has at most piece_cap spans
  int32_t* spans = (int32_t*)scratch_get(sizeof(int32_t) * 2 * (size_t)(a.piece_cap > 0 ? a.piece_cap : 1), a.stream);
  if (!spans) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  if (int rc = member_findall(h, b, n, d_piece_prefix, spans, a.piece_cap, a.stream, known_total, known_max)) return rc;
  a.d_spans = spans;
  return gather_enqueue(b, n, a);
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_gather_spans_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, const int64_t* d_prefix,
                         const int32_t* d_spans, int32_t row_pairs, int32_t pair, int64_t piece_cap, int64_t* d_owner,
                         int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                         void* stream) {
  return gather_run(csr(d_data, d_offsets), BATCH_CSR, n,
                    SpanArgs{{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_prefix, d_spans,
                             row_pairs, pair, piece_cap});
}
int mrx_gather_spans_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                                 const int64_t* d_prefix, const int32_t* d_spans, int32_t row_pairs, int32_t pair,
                                 int64_t piece_cap, int64_t* d_owner, int64_t* d_out_offsets, uint8_t* d_out_data,
                                 int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return gather_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n,
                    SpanArgs{{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, d_prefix, d_spans,
                             row_pairs, pair, piece_cap});
}
int mrx_gather_spans_batch(const uint8_t* data, const int64_t* offsets, int64_t n, const int64_t* prefix,
                           const int32_t* spans, int32_t row_pairs, int32_t pair, int64_t piece_cap, int64_t* owner,
                           int64_t* out_offsets, uint8_t* out_data, int64_t out_cap, int64_t* totals) {
  const HostOut o{owner, out_offsets, out_data, totals};
  if (int rc = host_out_check(n, piece_cap, out_cap, offsets, o)) return rc;
  if (row_pairs < 1) return internal_fail(MRX_E_ARGUMENT, "row_pairs must be >= 1");
  if (pair < 0 || pair >= row_pairs) return internal_fail(MRX_E_ARGUMENT, "pair must be in [0, row_pairs)");
  if (!prefix || (n > 0 && prefix[n] > 0 && !spans)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n > 0 && prefix[n] < 0) return internal_fail(MRX_E_ARGUMENT, "prefix[n] must be >= 0");
  DevBatch b; DevOut d; DevBuf<int64_t> pre; DevBuf<int32_t> sp;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  // the kernel reads the rows that fit: the spans buffer holds piece_cap rows at least
  const size_t rows = n > 0 ? (size_t)prefix[n] : 0, held = rows > (size_t)piece_cap ? rows : (size_t)piece_cap;
  if (int rc = pre.alloc((size_t)n + 1)) return rc;
  if (int rc = sp.alloc(held * 2 * (size_t)row_pairs)) return rc;
  if (int rc = d.alloc(piece_cap, out_cap)) return rc;
  MRX_HIP_TRY(hipMemcpy(pre.p, prefix, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice));
  if (rows) MRX_HIP_TRY(hipMemcpy(sp.p, spans, sizeof(int32_t) * 2 * (size_t)row_pairs * rows, hipMemcpyHostToDevice));
  int64_t tot[2] = {0, 0};
  const int rc = mrx_gather_spans_dev(b.data, b.offsets, n, pre.p, sp.p, row_pairs, pair, piece_cap, d.ow.p, d.oo.p, d.od.p,
                                      out_cap, d.dt.p, tot, nullptr);
  return d.copy_out(rc, tot, piece_cap, o);
}

int mrx_extract_dev(const mrx_handle* h, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                    int64_t* d_piece_prefix, int64_t* d_owner, int64_t* d_out_offsets, int64_t piece_cap,
                    uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return extract_run(h, csr(d_data, d_offsets), BATCH_CSR, n, -1, -1, d_piece_prefix,
                     SpanArgs{{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, nullptr, nullptr, 1,
                              0, piece_cap});
}
int mrx_extract_known_dev(const mrx_handle* h, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                          int64_t end_offset, int64_t max_text_len, int64_t* d_piece_prefix, int64_t* d_owner,
                          int64_t* d_out_offsets, int64_t piece_cap, uint8_t* d_out_data, int64_t out_cap,
                          int64_t* d_totals, int64_t* totals, void* stream) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return extract_run(h, csr(d_data, d_offsets), BATCH_CSR, n, end_offset, max_text_len, d_piece_prefix,
                     SpanArgs{{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, nullptr, nullptr, 1,
                              0, piece_cap});
}
int mrx_extract_strided_dev(const mrx_handle* h, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                            int64_t n, int64_t* d_piece_prefix, int64_t* d_owner, int64_t* d_out_offsets,
                            int64_t piece_cap, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals,
                            void* stream) {
  return extract_run(h, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1, -1, d_piece_prefix,
                     SpanArgs{{d_owner, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream}, nullptr, nullptr, 1,
                              0, piece_cap});
}
int mrx_extract_batch(const mrx_handle* h, const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* piece_prefix,
                      int64_t* owner, int64_t* out_offsets, int64_t piece_cap, uint8_t* out_data, int64_t out_cap,
                      int64_t* totals) {
  if (!h) return internal_fail(MRX_E_ARGUMENT, "null handle");
  const HostOut o{owner, out_offsets, out_data, totals};
  if (int rc = host_out_check(n, piece_cap, out_cap, offsets, o)) return rc;
  if (!piece_prefix) return internal_fail(MRX_E_ARGUMENT, "null argument");
  const std::string refused = handle_refusal(h);
  if (!refused.empty()) return internal_fail(MRX_E_UNSUPPORTED, refused);
  DevBatch b; DevOut d; DevBuf<int64_t> pre;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = pre.alloc((size_t)n + 1)) return rc;
  if (int rc = d.alloc(piece_cap, out_cap)) return rc;
  int64_t tot[2] = {0, 0};
  const int rc = mrx_extract_known_dev(h, b.data, b.offsets, n, b.nbytes, b.longest, pre.p, d.ow.p, d.oo.p, piece_cap, d.od.p,
                                       out_cap, d.dt.p, tot, nullptr);
  if (rc == MRX_OK || rc == MRX_E_CAPACITY)
    MRX_HIP_TRY(hipMemcpy(piece_prefix, pre.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost));
  return d.copy_out(rc, tot, piece_cap, o);
}

void mrx_debug_extract_grid(int workgroups) { g_extract_grid = workgroups > 0 ? workgroups : 0; }

}  // extern "C"
