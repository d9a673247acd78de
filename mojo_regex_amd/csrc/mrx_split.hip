// regex.split on the device (gfx950 / CDNA4): the text between successive findall matches.  The findall underneath
// and the prefix sums are mrx_kernels.hip's, reached through mrx_core.hpp.
#include <string>

#include "mrx_core.hpp"
#include "../../include/mrx_testing.h"

using namespace mrx;

namespace {
// ---- regex.split (matcher.mojo:1357-1393): the text between successive findall matches ------------------------
// kept[i] = min(matches of text i, maxsplit) (all of them for maxsplit == 0, none for a negative maxsplit)
__global__ __launch_bounds__(kBlock) void k_split_kept(int64_t n, const int64_t* __restrict__ prefix, int64_t maxsplit,
                                                       int32_t* __restrict__ kept) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = prefix[i + 1] - prefix[i];
    kept[i] = (int32_t)(maxsplit == 0 ? c : maxsplit < 0 ? 0 : (c < maxsplit ? c : maxsplit));
  }
}
// piece_prefix[i] = (kept matches of the texts before i) + i: text i yields kept[i] + 1 pieces
__global__ __launch_bounds__(kBlock) void k_split_prefix(int64_t n, const int64_t* __restrict__ kept_prefix,
                                                         int64_t* __restrict__ piece_prefix, int64_t* __restrict__ total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
    piece_prefix[i] = kept_prefix[i] + i;
    if (i == n && total) *total = kept_prefix[n] + n;
  }
}
// one lane per PIECE: piece q of text i is [end of match q - 1 (0 for q = 0), start of match q (the text's end behind the
// last kept match)); its text is found by bisection of the piece offsets (coalesced stores whatever the texts hold)
__global__ __launch_bounds__(kBlock) void k_split_pieces(Layout lay, int64_t n, const int64_t* __restrict__ prefix,
                                                         const int32_t* __restrict__ spans, const int64_t* __restrict__ piece_prefix,
                                                         int32_t* __restrict__ pieces, int64_t piece_cap) {
  const int64_t total = piece_prefix[n] < piece_cap ? piece_prefix[n] : piece_cap;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = n;   // the last i with piece_prefix[i] <= j
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (piece_prefix[mid] <= j) lo = mid; else hi = mid;
    }
    const int64_t i = lo, q = j - piece_prefix[i];
    const int64_t kept = piece_prefix[i + 1] - piece_prefix[i] - 1;
    const int32_t* sp = spans + 2 * prefix[i];
    const int a = q == 0 ? 0 : sp[2 * (q - 1) + 1];
    const int b = q < kept ? sp[2 * q] : lay.text(i).len;
    // exact-literal plans return overlapping spans (findall of a self-overlapping literal), so match q may begin
    // before match q-1 ends: that piece is empty, [a, a), never a reversed range
    *(int2*)(pieces + 2 * j) = make_int2(a, b > a ? b : a);
  }
}

int run_split(const mrx_handle* h, const Layout& lay, int64_t n, int64_t maxsplit, int64_t* d_piece_prefix, int32_t* d_pieces,
              int64_t piece_cap, int64_t* total, void* st) {
  hipStream_t s = (hipStream_t)st;
  ScratchScope scratch_scope_(s);
  if (!h) return internal_fail(MRX_E_ARGUMENT, "null handle");
  if (n < 0 || piece_cap < 0 || !d_piece_prefix || (!d_pieces && piece_cap > 0)) return internal_fail(MRX_E_ARGUMENT, "bad arguments");
  if ((uintptr_t)d_pieces & 7) return internal_fail(MRX_E_ARGUMENT, "d_pieces must be 8-byte aligned");
  // findall into scratch: every piece but a text's last ends at a match, so piece_cap holds the spans of any result
  // that fits (maxsplit == 0: pieces = spans + n)
  int64_t* d_prefix = nullptr;
  int32_t* d_spans = nullptr;
  int32_t* d_kept = nullptr;
  int64_t* d_kprefix = nullptr;
  int64_t* d_tot = nullptr;
  const int64_t span_cap = piece_cap > n ? piece_cap : n + 1;
  MRX_SCRATCH(d_prefix, sizeof(int64_t) * (n + 1), s);
  MRX_SCRATCH(d_spans, sizeof(int32_t) * 2 * (size_t)span_cap, s);
  MRX_SCRATCH(d_kept, sizeof(int32_t) * (n > 0 ? n : 1), s);
  MRX_SCRATCH(d_kprefix, sizeof(int64_t) * (n + 1), s);
  MRX_SCRATCH(d_tot, sizeof(int64_t) * 2, s);
  int64_t nspans = 0;
  int rc_f = run_findall(h, lay, n, d_prefix, d_spans, span_cap, &nspans, s);
  if (rc_f == MRX_E_CAPACITY && maxsplit == 0) {   // pieces = matches + n: the need is known
    if (total) *total = nspans + n;
    return internal_fail(MRX_E_CAPACITY, "piece buffer too small: need " + std::to_string(nspans + n));
  }
  if (rc_f == MRX_E_CAPACITY) {   // a limit is on: the pieces may well fit although the matches did not -- once more, all of them
    MRX_SCRATCH(d_spans, sizeof(int32_t) * 2 * (size_t)nspans, s);
    rc_f = run_findall(h, lay, n, d_prefix, d_spans, nspans, &nspans, s);
  }
  if (rc_f != MRX_OK) return rc_f;
  const char* scanned = mrx_last_kernel_name();
  if (n > 0) {
    hipLaunchKernelGGL(k_split_kept, dim3(device_grid(n, kBlock)), dim3(kBlock), 0, s, n, d_prefix, maxsplit, d_kept);
    if (int rc = device_scan<int32_t>(d_kept, n, d_kprefix, d_tot, s)) return rc;
  } else {
    MRX_HIP_TRY(hipMemsetAsync(d_kprefix, 0, sizeof(int64_t), s));
  }
  hipLaunchKernelGGL(k_split_prefix, dim3(device_grid(n + 1, kBlock)), dim3(kBlock), 0, s, n, d_kprefix, d_piece_prefix, d_tot + 1);
  int64_t pieces_total = 0;
  MRX_HIP_TRY(hipMemcpyAsync(&pieces_total, d_tot + 1, sizeof pieces_total, hipMemcpyDeviceToHost, s));
  MRX_HIP_TRY(hipStreamSynchronize(s));
  if (total) *total = pieces_total;
  if (piece_cap > 0 && n > 0)
    hipLaunchKernelGGL(k_split_pieces, dim3(device_grid(pieces_total < piece_cap ? pieces_total : piece_cap, kBlock)), dim3(kBlock), 0, s,
                       lay, n, d_prefix, d_spans, d_piece_prefix, d_pieces, piece_cap);
  MRX_HIP_TRY(hipGetLastError());
  set_last_kernel(scanned);   // (the scan that found the separators)
  if (pieces_total > piece_cap) return internal_fail(MRX_E_CAPACITY, "piece buffer too small: need " + std::to_string(pieces_total));
  return MRX_OK;
}
}  // namespace
extern "C" {
int mrx_split_dev(const mrx_handle* h, const uint8_t* d, const int64_t* off, int64_t n, int64_t maxsplit,
                  int64_t* d_piece_prefix, int32_t* d_pieces, int64_t piece_cap, int64_t* total, void* st) {
  return run_split(h, csr(d, off), n, maxsplit, d_piece_prefix, d_pieces, piece_cap, total, st);
}
int mrx_split_strided_dev(const mrx_handle* h, const uint8_t* d, int64_t stride, const int32_t* lens, int32_t len, int64_t n,
                          int64_t maxsplit, int64_t* d_piece_prefix, int32_t* d_pieces, int64_t piece_cap, int64_t* total, void* st) {
  const TextBatch b = strided(d, stride, lens, len);
  if (int rc = check_batch(b, BATCH_PITCH)) return rc;
  return run_split(h, b, n, maxsplit, d_piece_prefix, d_pieces, piece_cap, total, st);
}
int mrx_split_batch(const mrx_handle* h, const uint8_t* data, const int64_t* off, int64_t n, int64_t maxsplit,
                    int64_t* piece_prefix, int32_t* pieces, int64_t piece_cap, int64_t* total) {
  DevBatch b; DevBuf<int64_t> pre; DevBuf<int32_t> pc;
  if (int rc = b.upload(data, off, n)) return rc;
  if (int rc = pre.alloc(n + 1)) return rc;
  if (int rc = pc.alloc(2 * (size_t)(piece_cap > 0 ? piece_cap : 1))) return rc;
  int64_t tot = 0;
  const int rc = mrx_split_dev(h, b.data, b.offsets, n, maxsplit, pre.p, pc.p, piece_cap, &tot, nullptr);
  if (total) *total = tot;
  if (rc != MRX_OK) return rc;
  MRX_HIP_TRY(hipMemcpy(piece_prefix, pre.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost));
  if (tot > 0) MRX_HIP_TRY(hipMemcpy(pieces, pc.p, sizeof(int32_t) * 2 * tot, hipMemcpyDeviceToHost));
  return MRX_OK;
}
}  // extern "C"
