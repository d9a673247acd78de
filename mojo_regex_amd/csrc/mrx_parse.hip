// Numbers (include/mrx.h, "numbers"): whole texts, or the bytes under spans of texts, parsed to int64 or float64 where
// they lie.  One kernel, k_parse, a lane per row; no scratch, no atomics, nothing read back unless the caller passes a
// host `totals`.
//
// Route.  The whole-text form is the kernel without a row CSR: row r is text r.  With spans, rows =
// d_prefix[n] is read on the device; a lane finds its row's text in the row CSR, clamps the pair as k_extract_sizes
// does and parses text[s' .. e') through parse_piece (mrx_parse_bits.hpp), which loads the aligned 16-byte words of
// the piece and nothing else.  A wavefront takes a contiguous run of rows, 64 a round, so the stores of a round -- one
// int64, one status byte and optionally one owner per lane -- are each coalesced.  The text of a row is found by the
// plain per-lane bisection of k_extract_sizes: the lanes of a round ask for neighbouring rows, so all but the last
// steps of their searches load the same words.  Narrowing the search per wavefront as k_extract_gather does (one
// bisection for the run's first row, a gallop per round, lanes bisecting in between) measured slower: 0.061 against
// 0.049 ms on 2^20 rows of one per text, no difference on 38 M rows (profiles/parse.md).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_gather_bits.hpp"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_parse_bits.hpp"

namespace mrx {
namespace {

constexpr int kParseBlock = 256;
constexpr unsigned kParseMaxGrid = 2048;   // 8 workgroups per CU, as extract; the kernel strides over what is left

std::atomic<int> g_parse_grid{0};   // mrx_debug_parse_grid(): workgroups at most (0 = no cap of its own)

// the rows: null prefix = the whole-text form (row r is text r, and none of the other fields is read)
struct ParseRows {
  const int64_t* prefix;
  const int32_t* spans;
  int32_t row_pairs, pair;
  int64_t row_cap;
  int64_t* owner;
  int64_t* totals;
};

__global__ __launch_bounds__(kParseBlock) void k_parse(const TextBatch B, int64_t n, const ParseRows R, int kind,
                                                       int64_t fill, int64_t* __restrict__ values,
                                                       uint8_t* __restrict__ status) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (kParseBlock / 64), w = (int64_t)blockIdx.x * (kParseBlock / 64) + ((int)threadIdx.x >> 6);
  int64_t rows = n;
  if (R.prefix) {
    rows = R.prefix[n];
    if (w == 0 && lane == 0) R.totals[0] = rows;
    if (rows > R.row_cap) return;
  }
  // a wavefront takes a contiguous run of rows, 64 a round
  const int64_t per = ((rows + nw - 1) / nw + 63) & ~(int64_t)63;
  const int64_t r_begin = w * per, r_end = r_begin + per < rows ? r_begin + per : rows;
  if (r_begin >= r_end) return;
  for (int64_t r = r_begin + lane; r < r_end; r += 64) {
    int64_t i = r;
    int32_t s = 0, e = 0x7fffffff;
    if (R.prefix) {
      i = gather_last_le(R.prefix, 0, n, r);   // prefix[i] <= r < prefix[i + 1]: texts without rows are passed
      const int2 se = *(const int2*)(R.spans + 2 * (r * R.row_pairs + R.pair));
      s = se.x;
      e = se.y;
    }
    int32_t L;
    const uint8_t* tp = B.text(i, &L);
    s = s < 0 ? 0 : s < L ? s : L;
    e = e < s ? s : e < L ? e : L;
    uint64_t bits = 0;
    const int st = parse_piece(tp + s, (int64_t)(e - s), kind, &bits);
    values[r] = st == MRX_NUM_OK ? (int64_t)bits : fill;
    status[r] = (uint8_t)st;
    if (R.owner) R.owner[r] = i;
  }
}

unsigned parse_grid(int64_t rows) {
  int64_t g = (rows + kParseBlock - 1) / kParseBlock;
  g = g < 1 ? 1 : g > (int64_t)kParseMaxGrid ? (int64_t)kParseMaxGrid : g;
  const int capped = g_parse_grid.load(std::memory_order_relaxed);
  return (unsigned)(capped > 0 && g > capped ? capped : g);
}

struct ParseOut {
  int32_t kind;
  int64_t fill;
  int64_t* d_values;
  uint8_t* d_status;
  void* stream;
};

int kind_check(int32_t kind) {
  if (kind != MRX_NUM_INT10 && kind != MRX_NUM_INT16 && kind != MRX_NUM_FLOAT)
    return internal_fail(MRX_E_ARGUMENT, "kind must be MRX_NUM_INT10, MRX_NUM_INT16 or MRX_NUM_FLOAT");
  return MRX_OK;
}

int launch(const TextBatch& b, int64_t n, const ParseRows& r, int64_t lanes, const ParseOut& o) {
  hipLaunchKernelGGL(k_parse, dim3(parse_grid(lanes)), dim3(kParseBlock), 0, (hipStream_t)o.stream, b, n, r, (int)o.kind,
                     o.fill, o.d_values, o.d_status);
  MRX_HIP_TRY(hipGetLastError());
  set_last_kernel("k_parse");
  return MRX_OK;
}

// argument errors: nothing has touched the device when one of them returns
int parse_run(const TextBatch& b, BatchForm form, int64_t n, const ParseOut& o) {
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (int rc = kind_check(o.kind)) return rc;
  if (int rc = check_batch(b, form)) return rc;
  if (n > 0 && (!o.d_values || !o.d_status)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n == 0) return MRX_OK;
  return launch(b, n, ParseRows{nullptr, nullptr, 1, 0, 0, nullptr, nullptr}, n, o);
}

int parse_spans_run(const TextBatch& b, BatchForm form, int64_t n, const ParseRows& r, int64_t* totals, const ParseOut& o) {
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (r.row_cap < 0) return internal_fail(MRX_E_ARGUMENT, "row_cap must be >= 0");
  if (int rc = kind_check(o.kind)) return rc;
  if (r.row_pairs < 1) return internal_fail(MRX_E_ARGUMENT, "row_pairs must be >= 1");
  if (r.pair < 0 || r.pair >= r.row_pairs) return internal_fail(MRX_E_ARGUMENT, "pair must be in [0, row_pairs)");
  if ((uintptr_t)r.spans & 7) return internal_fail(MRX_E_ARGUMENT, "d_spans must be 8-byte aligned");
  if (int rc = check_batch(b, form)) return rc;
  if (!r.prefix || !r.totals || (r.row_cap > 0 && (!r.spans || !o.d_values || !o.d_status)))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  hipStream_t hs = (hipStream_t)o.stream;
  if (n == 0) {
    MRX_HIP_TRY(hipMemsetAsync(r.totals, 0, sizeof(int64_t), hs));
    if (totals) totals[0] = 0;
    set_last_kernel("k_parse");
    return MRX_OK;
  }
  if (int rc = launch(b, n, r, r.row_cap, o)) return rc;   // (rows that fit are at most row_cap)
  if (!totals) return MRX_OK;
  MRX_HIP_TRY(hipMemcpyAsync(totals, r.totals, sizeof(int64_t), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));
  if (totals[0] > r.row_cap)
    return internal_fail(MRX_E_CAPACITY, "row buffers too small: need " + std::to_string(totals[0]));
  return MRX_OK;
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_parse_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int32_t kind, int64_t fill,
                  int64_t* d_values, uint8_t* d_status, void* stream) {
  return parse_run(csr(d_data, d_offsets), BATCH_CSR, n, ParseOut{kind, fill, d_values, d_status, stream});
}
int mrx_parse_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                          int32_t kind, int64_t fill, int64_t* d_values, uint8_t* d_status, void* stream) {
  return parse_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n, ParseOut{kind, fill, d_values, d_status, stream});
}
int mrx_parse_spans_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t n, const int64_t* d_prefix,
                        const int32_t* d_spans, int32_t row_pairs, int32_t pair, int32_t kind, int64_t fill,
                        int64_t row_cap, int64_t* d_values, uint8_t* d_status, int64_t* d_owner, int64_t* d_totals,
                        int64_t* totals, void* stream) {
  return parse_spans_run(csr(d_data, d_offsets), BATCH_CSR, n,
                         ParseRows{d_prefix, d_spans, row_pairs, pair, row_cap, d_owner, d_totals}, totals,
                         ParseOut{kind, fill, d_values, d_status, stream});
}
int mrx_parse_spans_strided_dev(const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                                const int64_t* d_prefix, const int32_t* d_spans, int32_t row_pairs, int32_t pair,
                                int32_t kind, int64_t fill, int64_t row_cap, int64_t* d_values, uint8_t* d_status,
                                int64_t* d_owner, int64_t* d_totals, int64_t* totals, void* stream) {
  return parse_spans_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n,
                         ParseRows{d_prefix, d_spans, row_pairs, pair, row_cap, d_owner, d_totals}, totals,
                         ParseOut{kind, fill, d_values, d_status, stream});
}

int mrx_parse_batch(const uint8_t* data, const int64_t* offsets, int64_t n, int32_t kind, int64_t fill, int64_t* values,
                    uint8_t* status) {
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (int rc = kind_check(kind)) return rc;
  if (!offsets || (n > 0 && (!values || !status))) return internal_fail(MRX_E_ARGUMENT, "null argument");
  DevBatch b; DevBuf<int64_t> dv; DevBuf<uint8_t> ds;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n == 0) return MRX_OK;
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = dv.alloc((size_t)n)) return rc;
  if (int rc = ds.alloc((size_t)n)) return rc;
  if (int rc = mrx_parse_dev(b.data, b.offsets, n, kind, fill, dv.p, ds.p, nullptr)) return rc;
  MRX_HIP_TRY(hipMemcpy(values, dv.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost));
  MRX_HIP_TRY(hipMemcpy(status, ds.p, (size_t)n, hipMemcpyDeviceToHost));
  return MRX_OK;
}

void mrx_debug_parse_grid(int workgroups) { g_parse_grid = workgroups > 0 ? workgroups : 0; }

}  // extern "C"
