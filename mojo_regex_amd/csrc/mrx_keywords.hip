// Keywords (include/mrx.h, "keywords"): one Aho-Corasick automaton over all entries of a keyword set, one pass over the
// texts.  The automaton, the piece decomposition and the walk are in mrx_kw_bits.hpp, the handle and what the kernels
// share with leftmost and sub (mrx_kw_sub.hip) in mrx_kw_dev.hpp; here are the launches and the entry points.
//
//   k_kw_pieces    (CSR) ceil(len / P) per text; the existing exclusive scan makes the first piece of every text of it
//   k_kw_count     a lane walks a piece and writes its hit count
//   exclusive_scan over the pieces' counts: scan[npieces + 1]
//   k_kw_text      per text, from the scan at the text's first piece and at the next text's: contains, count, the text
//                  prefix of findall, or filter's flags
//   k_kw_emit      (findall, behind the one synchronisation for the total) walks the pieces that have hits again and
//                  writes entries and spans at scan[piece], clamped at span_cap
// Pieces are numbered text-major.  Fixed pitch: every text has ceil(longest / P) of them (1 at least), so piece -> text is
// a division.  CSR: a bisection of the texts' first pieces; the grid is sized by an upper bound of the piece count
// (bytes / P + n), and the pieces beyond the last text's do nothing.
//
// The per-byte path is a dependent load, next = table[state * ncls + cls[byte]].  The rows of the first states (the
// shallowest: where a walk over text without hits lives) are copied into LDS beside the class map by every workgroup,
// as many as fit kKwTierWords; deeper rows are read from global memory.  No atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"
#include "mrx_kw_bits.hpp"
#include "mrx_kw_dev.hpp"

namespace mrx {
namespace {

constexpr uint32_t kKwFilterFlags = MRX_FILTER_INVERT | MRX_FILTER_ALL;

std::atomic<int64_t> g_kw_piece{0};
std::atomic<int> g_kw_lds{1};

std::string kw_describe_text(int64_t m, int64_t distinct, int32_t states, int32_t ncls, int32_t lmax, uint32_t flags) {
  char buf[256];
  snprintf(buf, sizeof buf, "keywords: m=%lld distinct=%lld states=%d classes=%d lmax=%d table_bytes=%lld ignore_case=%d",
           (long long)m, (long long)distinct, states, ncls, lmax, (long long)states * ncls * 4,
           (flags & MRX_KW_IGNORE_CASE) ? 1 : 0);
  return buf;
}
size_t copy_text(const std::string& s, char* buf, size_t cap) {
  if (buf && cap) {
    const size_t k = s.size() < cap - 1 ? s.size() : cap - 1;
    memcpy(buf, s.data(), k);
    buf[k] = 0;
  }
  return s.size();
}

__device__ __forceinline__ KwJob kw_piece_job(const TextBatch& B, int64_t n, const KwPieces& pc, int32_t lmax, int64_t piece) {
  int64_t i, lp;
  if (!kw_piece_text(pc, n, piece, &i, &lp)) return kw_no_job();
  int32_t L = 0;
  const uint8_t* tp = B.text(i, &L);
  return kw_job(tp, L, lp, pc.P, lmax);
}

// EMIT false: out[piece] = the piece's hit count.  EMIT true: scan[piece] is where the piece's hits go.
template <bool EMIT>
__device__ __forceinline__ void kw_pass(const TextBatch& B, int64_t n, const KwView& V, const KwPieces& pc, int64_t* __restrict__ out,
                                        const int64_t* __restrict__ scan, int32_t* __restrict__ entries, int32_t* __restrict__ spans,
                                        int64_t cap) {
  const KwDevTab tab = kw_stage_tier(V);
  const int64_t nthreads = (int64_t)gridDim.x * kKwBlock;
  for (int64_t piece = (int64_t)blockIdx.x * kKwBlock + threadIdx.x; piece < pc.npieces; piece += nthreads) {
    if constexpr (EMIT) {
      KwEmitSink sink{V.meta, entries, spans, cap, scan[piece]};
      if (scan[piece + 1] == sink.pos) continue;   // (a piece without hits is not walked again)
      kw_walk(tab, kw_piece_job(B, n, pc, V.lmax, piece), sink);
    } else {
      KwCountSink sink{V.meta, 0};
      kw_walk(tab, kw_piece_job(B, n, pc, V.lmax, piece), sink);
      out[piece] = sink.cnt;
    }
  }
}

__global__ __launch_bounds__(kKwBlock) void k_kw_count(const TextBatch B, int64_t n, const KwView V, const KwPieces pc,
                                                       int64_t* __restrict__ cnt) {
  kw_pass<false>(B, n, V, pc, cnt, nullptr, nullptr, nullptr, 0);
}
__global__ __launch_bounds__(kKwBlock) void k_kw_emit(const TextBatch B, int64_t n, const KwView V, const KwPieces pc,
                                                      const int64_t* __restrict__ scan, int32_t* __restrict__ entries,
                                                      int32_t* __restrict__ spans, int64_t cap) {
  kw_pass<true>(B, n, V, pc, nullptr, scan, entries, spans, cap);
}

__global__ __launch_bounds__(256) void k_kw_pieces(const TextBatch B, int64_t n, int64_t P, int64_t* __restrict__ per) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t L = 0;
    (void)B.text(i, &L);
    per[i] = ((int64_t)L + P - 1) / P;
  }
}

// what k_kw_text writes: the one that is not null
struct KwTextOut {
  uint8_t* flag;     // contains
  int64_t* count;    // count
  int64_t* prefix;   // findall: [n + 1]
  int64_t* klen;     // filter: the kept length and the keep flag of every text
  int64_t* keep;
  uint32_t filter_flags;
};
__global__ __launch_bounds__(256) void k_kw_text(const TextBatch B, int64_t n, const KwPieces pc, const int64_t* __restrict__ scan,
                                                 const KwTextOut o) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = pc.first ? pc.first[i] : i * pc.per_text, b = pc.first ? pc.first[i + 1] : a + pc.per_text;
    a = a < pc.npieces ? a : pc.npieces;   // (only bounds that were too small can put a text's pieces behind the scan)
    b = b < pc.npieces ? b : pc.npieces;
    const int64_t at = scan[a], hits = scan[b] - at;
    if (o.flag) o.flag[i] = hits > 0 ? 1 : 0;
    if (o.count) o.count[i] = hits;
    if (o.prefix) {
      o.prefix[i] = at;
      if (i == n - 1) o.prefix[n] = at + hits;
    }
    if (o.klen) {
      const bool kp = (hits > 0) != ((o.filter_flags & MRX_FILTER_INVERT) != 0);
      int32_t L = 0;
      (void)B.text(i, &L);
      o.klen[i] = kp ? (int64_t)L : 0;
      o.keep[i] = kp ? 1 : 0;
    }
  }
}

struct KwRun {
  KwView view;
  KwPieces pc;
  int64_t* scan = nullptr;    // [npieces + 1]
  int64_t* d_total = nullptr;
  unsigned grid = 1;
};

// The first half of every operation on a checked batch of n >= 1 texts, inside the caller's ScratchScope: the pieces,
// their counts and the scan.  known_total / known_max: a CSR batch's bounds (< 0: read back, one synchronisation).
int kw_count_pieces(const mrx_kw* k, const TextBatch& b, int64_t n, int64_t known_total, int64_t known_max, KwRun& r, void* st) {
  hipStream_t hs = (hipStream_t)st;
  KwPieces& pc = r.pc;
  if (int rc = kw_plan_pieces(k->lmax, b, n, known_total, known_max, pc, st)) return rc;
  r.view = kw_view(k->fwd, k->lmax);
  r.grid = grid_for(pc.npieces, kKwBlock, kKwMaxGrid);
  int64_t* cnt = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)pc.npieces, st);
  r.scan = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(pc.npieces + 1), st);
  r.d_total = (int64_t*)scratch_get(sizeof(int64_t), st);
  if (!cnt || !r.scan || !r.d_total) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  void* timer = scan_timer_begin(st);
  hipLaunchKernelGGL(k_kw_count, dim3(r.grid), dim3(kKwBlock), 0, hs, b, n, r.view, r.pc, cnt);
  scan_timer_end(timer);
  MRX_HIP_TRY(hipGetLastError());
  set_last_kernel("k_kw_count");
  return exclusive_scan(cnt, pc.npieces, r.scan, r.d_total, st);
}

int kw_text_pass(const TextBatch& b, int64_t n, const KwRun& r, const KwTextOut& o, hipStream_t hs) {
  hipLaunchKernelGGL(k_kw_text, dim3(grid_for(n, 256, 4096)), dim3(256), 0, hs, b, n, r.pc, r.scan, o);
  MRX_HIP_TRY(hipGetLastError());
  return MRX_OK;
}

// contains (d_flag) or count (d_count): one of the two is not null
int kw_per_text(const mrx_kw* k, const TextBatch& b, BatchForm form, int64_t n, uint8_t* d_flag, int64_t* d_count, void* st) {
  if (!k) return internal_fail(MRX_E_ARGUMENT, "null keyword set");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (n > 0 && !d_flag && !d_count) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n == 0) return MRX_OK;
  ScratchScope scope_(st);
  KwRun r;
  if (int rc = kw_count_pieces(k, b, n, -1, -1, r, st)) return rc;
  return kw_text_pass(b, n, r, KwTextOut{d_flag, d_count, nullptr, nullptr, nullptr, 0}, (hipStream_t)st);
}

int kw_findall(const mrx_kw* k, const TextBatch& b, BatchForm form, int64_t n, int64_t known_total, int64_t known_max,
               int64_t* d_text_prefix, int32_t* d_entries, int32_t* d_spans, int64_t span_cap, int64_t* total, void* st) {
  if (!k) return internal_fail(MRX_E_ARGUMENT, "null keyword set");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
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
  KwRun r;
  if (int rc = kw_count_pieces(k, b, n, known_total, known_max, r, st)) return rc;
  if (int rc = kw_text_pass(b, n, r, KwTextOut{nullptr, nullptr, d_text_prefix, nullptr, nullptr, 0}, hs)) return rc;
  int64_t tot = 0;
  MRX_HIP_TRY(hipMemcpyAsync(&tot, r.d_total, sizeof(int64_t), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));   // the one synchronisation: the total
  if (total) *total = tot;
  if (tot > span_cap) return internal_fail(MRX_E_CAPACITY, "span buffer too small: need " + std::to_string(tot));
  if (tot == 0) return MRX_OK;
  hipLaunchKernelGGL(k_kw_emit, dim3(r.grid), dim3(kKwBlock), 0, hs, b, n, r.view, r.pc, r.scan, d_entries, d_spans, span_cap);
  MRX_HIP_TRY(hipGetLastError());
  set_last_kernel("k_kw_emit");
  return MRX_OK;
}

int kw_filter(const mrx_kw* k, uint32_t flags, const TextBatch& b, BatchForm form, int64_t n, int64_t known_total,
              int64_t known_max, const PackedDest& o) {
  if (!k) return internal_fail(MRX_E_ARGUMENT, "null keyword set");
  if (flags & ~kKwFilterFlags) return internal_fail(MRX_E_ARGUMENT, "unknown flag bits");
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (o.out_cap < 0) return internal_fail(MRX_E_ARGUMENT, "out_cap must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (!o.d_out_offsets || !o.d_totals || (n > 0 && !o.d_rows) || (o.out_cap > 0 && !o.d_out_data))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n == 0) return filter_no_text(b, known_max, o);
  ScratchScope scope_(o.stream);
  int64_t* klen = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, o.stream);
  int64_t* keep = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, o.stream);
  int64_t* pos = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), o.stream);
  int64_t* rank = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), o.stream);
  if (!klen || !keep || !pos || !rank) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
  KwRun r;
  if (int rc = kw_count_pieces(k, b, n, known_total, known_max, r, o.stream)) return rc;
  if (int rc = kw_text_pass(b, n, r, KwTextOut{nullptr, nullptr, nullptr, klen, keep, flags}, (hipStream_t)o.stream)) return rc;
  return filter_compact(b, n, known_max, FilterWork{klen, keep, pos, rank}, o);
}

}  // namespace

int64_t kw_pinned_piece() { return g_kw_piece.load(); }

KwView kw_view(const mrx_kw_tables& t, int32_t lmax) {
  int64_t tier = g_kw_lds.load() ? kKwTierWords / t.ncls : 0;
  if (tier > t.states) tier = t.states;
  return KwView{t.table, t.cls, t.meta, t.ncls, lmax, (uint32_t)tier};
}

int kw_plan_pieces(int32_t lmax, const TextBatch& b, int64_t n, int64_t known_total, int64_t known_max, KwPieces& pc, void* st) {
  hipStream_t hs = (hipStream_t)st;
  int64_t bytes;
  if (b.offsets) {
    int64_t km = known_max;
    bytes = known_total;
    if (bytes < 0 || km < 0)
      if (int rc = batch_bounds(b.offsets, n, st, &bytes, &km)) return rc;
  } else {
    bytes = n * b.pitch_longest();
  }
  const int64_t pinned = g_kw_piece.load();
  pc.P = pinned > 0 ? pinned : kw_piece_rule(lmax, bytes);
  pc.first = nullptr;
  pc.per_text = 0;
  if (b.offsets) {
    int64_t* per = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)n, st);
    int64_t* first = (int64_t*)scratch_get(sizeof(int64_t) * (size_t)(n + 1), st);
    int64_t* unused = (int64_t*)scratch_get(sizeof(int64_t), st);
    if (!per || !first || !unused) return internal_fail(MRX_E_NO_DEVICE, "scratch allocation failed");
    hipLaunchKernelGGL(k_kw_pieces, dim3(grid_for(n, 256, 4096)), dim3(256), 0, hs, b, n, pc.P, per);
    MRX_HIP_TRY(hipGetLastError());
    if (int rc = exclusive_scan(per, n, first, unused, st)) return rc;
    pc.first = first;
    pc.npieces = bytes / pc.P + n;   // ceil(len / P) <= len / P + 1 for every text
  } else {
    pc.per_text = (b.pitch_longest() + pc.P - 1) / pc.P;
    if (pc.per_text < 1) pc.per_text = 1;
    pc.npieces = n * pc.per_text;
  }
  return MRX_OK;
}

// the checks that both builds share, and the automaton on the host
int kw_build_host(const uint8_t* data, const int64_t* offsets, int64_t m, uint32_t flags, KwAutomaton* A) {
  std::string err;
  if (int rc = kw_build(data, offsets, m, flags, A, &err)) return internal_fail(rc, err);
  return MRX_OK;
}
int kw_check_build(int64_t m, uint32_t flags, const void* offsets, const void* out) {
  if (m < 0) return internal_fail(MRX_E_ARGUMENT, "m must be >= 0");
  if (flags & ~(uint32_t)MRX_KW_IGNORE_CASE) return internal_fail(MRX_E_ARGUMENT, "unknown flag bits");
  if (!out || !offsets) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (m >= ((int64_t)1 << 31)) return internal_fail(MRX_E_ARGUMENT, "m must be below 2^31: a state keeps an entry's index in 32 bits");
  return MRX_OK;
}

int kw_upload_tables(const KwAutomaton& A, void* stream, mrx_kw_tables* t) {
  hipStream_t hs = (hipStream_t)stream;
  t->states = A.states;
  t->ncls = A.ncls;
  MRX_HIP_TRY(hipMalloc((void**)&t->table, sizeof(uint32_t) * A.table.size()));
  MRX_HIP_TRY(hipMalloc((void**)&t->cls, 256));
  MRX_HIP_TRY(hipMalloc((void**)&t->meta, sizeof(KwMeta) * A.meta.size()));
  MRX_HIP_TRY(hipMemcpyAsync(t->table, A.table.data(), sizeof(uint32_t) * A.table.size(), hipMemcpyHostToDevice, hs));
  MRX_HIP_TRY(hipMemcpyAsync(t->cls, A.cls.data(), 256, hipMemcpyHostToDevice, hs));
  MRX_HIP_TRY(hipMemcpyAsync(t->meta, A.meta.data(), sizeof(KwMeta) * A.meta.size(), hipMemcpyHostToDevice, hs));
  return MRX_OK;
}

namespace {

// the handle of a built automaton; data / offsets: the caller's entries on the host, kept folded for the reversed build
int kw_upload(const KwAutomaton& A, const uint8_t* data, const int64_t* offsets, void* stream, mrx_kw** out) {
  hipStream_t hs = (hipStream_t)stream;
  mrx_kw* k = new mrx_kw();
  struct Guard {   // the handle goes back on every early way out
    mrx_kw* k;
    ~Guard() { delete k; }
  } guard{k};
  k->m = A.m;
  k->distinct = A.distinct;
  k->lmax = A.lmax;
  k->flags = A.flags;
  k->entry_off.assign((size_t)A.m + 1, 0);
  for (int64_t j = 0; j <= A.m && A.m > 0; ++j) k->entry_off[(size_t)j] = offsets[j] - offsets[0];
  k->entry_data.resize((size_t)k->entry_off[(size_t)A.m]);
  for (size_t q = 0; q < k->entry_data.size(); ++q) {
    uint8_t c = data[offsets[0] + (int64_t)q];
    if ((A.flags & MRX_KW_IGNORE_CASE) && c >= 'A' && c <= 'Z') c |= 0x20;
    k->entry_data[q] = c;
  }
  if (int rc = kw_upload_tables(A, stream, &k->fwd)) return rc;
  MRX_HIP_TRY(hipStreamSynchronize(hs));   // the automaton's host copy goes with this call
  guard.k = nullptr;
  *out = k;
  return MRX_OK;
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_kw_build(const uint8_t* data, const int64_t* offsets, int64_t m, uint32_t flags, void* stream, mrx_kw** out) {
  if (int rc = kw_check_build(m, flags, offsets, out)) return rc;
  if (m > 0 && offsets[m] > offsets[0] && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  KwAutomaton A;
  if (int rc = kw_build_host(data, offsets, m, flags, &A)) return rc;
  return kw_upload(A, data, offsets, stream, out);
}
int mrx_kw_build_dev(const uint8_t* d_data, const int64_t* d_offsets, int64_t m, uint32_t flags, void* stream, mrx_kw** out) {
  if (int rc = kw_check_build(m, flags, d_offsets, out)) return rc;
  hipStream_t hs = (hipStream_t)stream;
  std::vector<int64_t> off((size_t)m + 1, 0);
  MRX_HIP_TRY(hipMemcpyAsync(off.data(), d_offsets, sizeof(int64_t) * off.size(), hipMemcpyDeviceToHost, hs));
  MRX_HIP_TRY(hipStreamSynchronize(hs));
  const int64_t bytes = off[(size_t)m] - off[0];
  if (bytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (bytes > 0 && !d_data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  std::vector<uint8_t> data((size_t)bytes);
  if (bytes > 0) {
    MRX_HIP_TRY(hipMemcpyAsync(data.data(), d_data + off[0], (size_t)bytes, hipMemcpyDeviceToHost, hs));
    MRX_HIP_TRY(hipStreamSynchronize(hs));
  }
  const int64_t base = off[0];
  for (int64_t& o : off) o -= base;
  KwAutomaton A;
  if (int rc = kw_build_host(data.data(), off.data(), m, flags, &A)) return rc;
  return kw_upload(A, data.data(), off.data(), stream, out);
}
void mrx_kw_free(mrx_kw* k) { delete k; }
int64_t mrx_kw_size(const mrx_kw* k) { return k ? k->m : 0; }
int64_t mrx_kw_distinct(const mrx_kw* k) { return k ? k->distinct : 0; }
size_t mrx_kw_describe(const mrx_kw* k, char* buf, size_t cap) {
  if (!k) return copy_text("keywords: null", buf, cap);
  return copy_text(kw_describe_text(k->m, k->distinct, k->fwd.states, k->fwd.ncls, k->lmax, k->flags), buf, cap);
}

int mrx_kw_contains_dev(const mrx_kw* k, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, uint8_t* d_flag,
                        void* stream) {
  return kw_per_text(k, csr(d_data, d_offsets), BATCH_CSR, n, d_flag, nullptr, stream);
}
int mrx_kw_contains_strided_dev(const mrx_kw* k, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                                int64_t n, uint8_t* d_flag, void* stream) {
  return kw_per_text(k, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, d_flag, nullptr, stream);
}
int mrx_kw_count_dev(const mrx_kw* k, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_count,
                     void* stream) {
  return kw_per_text(k, csr(d_data, d_offsets), BATCH_CSR, n, nullptr, d_count, stream);
}
int mrx_kw_count_strided_dev(const mrx_kw* k, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                             int64_t n, int64_t* d_count, void* stream) {
  return kw_per_text(k, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, nullptr, d_count, stream);
}

int mrx_kw_findall_dev(const mrx_kw* k, const uint8_t* d_data, const int64_t* d_offsets, int64_t n, int64_t* d_text_prefix,
                       int32_t* d_entries, int32_t* d_spans, int64_t span_cap, int64_t* total, void* stream) {
  return kw_findall(k, csr(d_data, d_offsets), BATCH_CSR, n, -1, -1, d_text_prefix, d_entries, d_spans, span_cap, total, stream);
}
int mrx_kw_findall_known_dev(const mrx_kw* k, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                             int64_t end_offset, int64_t max_text_len, int64_t* d_text_prefix, int32_t* d_entries,
                             int32_t* d_spans, int64_t span_cap, int64_t* total, void* stream) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return kw_findall(k, csr(d_data, d_offsets), BATCH_CSR, n, end_offset, max_text_len, d_text_prefix, d_entries, d_spans,
                    span_cap, total, stream);
}
int mrx_kw_findall_strided_dev(const mrx_kw* k, const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len,
                               int64_t n, int64_t* d_text_prefix, int32_t* d_entries, int32_t* d_spans, int64_t span_cap,
                               int64_t* total, void* stream) {
  return kw_findall(k, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1, -1, d_text_prefix, d_entries, d_spans,
                    span_cap, total, stream);
}

int mrx_kw_filter_dev(const mrx_kw* k, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                      int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals,
                      int64_t* totals, void* stream) {
  return kw_filter(k, flags, csr(d_data, d_offsets), BATCH_CSR, n, -1, -1,
                   PackedDest{d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream});
}
int mrx_kw_filter_known_dev(const mrx_kw* k, uint32_t flags, const uint8_t* d_data, const int64_t* d_offsets, int64_t n,
                            int64_t end_offset, int64_t max_text_len, int64_t* d_kept_idx, int64_t* d_out_offsets,
                            uint8_t* d_out_data, int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  if (end_offset < 0 || max_text_len < 0)
    return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must not be negative");
  return kw_filter(k, flags, csr(d_data, d_offsets), BATCH_CSR, n, end_offset, max_text_len,
                   PackedDest{d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream});
}
int mrx_kw_filter_strided_dev(const mrx_kw* k, uint32_t flags, const uint8_t* d_data, int64_t stride, const int32_t* d_lens,
                              int32_t len, int64_t n, int64_t* d_kept_idx, int64_t* d_out_offsets, uint8_t* d_out_data,
                              int64_t out_cap, int64_t* d_totals, int64_t* totals, void* stream) {
  return kw_filter(k, flags, strided(d_data, stride, d_lens, len), BATCH_PITCH, n, -1, -1,
                   PackedDest{d_kept_idx, d_out_offsets, d_out_data, out_cap, d_totals, totals, stream});
}

// host buffers: argument errors before any device work, as the _dev entry points
int mrx_kw_findall_batch(const mrx_kw* k, const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* text_prefix,
                         int32_t* entries, int32_t* spans, int64_t span_cap, int64_t* total) {
  if (!k || n < 0 || !offsets || !text_prefix || (span_cap > 0 && (!entries || !spans)))
    return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (span_cap < 0) return internal_fail(MRX_E_ARGUMENT, "span_cap must be >= 0");
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
  const int rc = mrx_kw_findall_known_dev(k, b.data, b.offsets, n, b.nbytes, b.longest, pre.p, en.p, (int32_t*)sp.p, span_cap,
                                          &tot, nullptr);
  if (total) *total = tot;
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  MRX_HIP_TRY(hipMemcpy(text_prefix, pre.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot > 0) {
    MRX_HIP_TRY(hipMemcpy(entries, en.p, sizeof(int32_t) * (size_t)tot, hipMemcpyDeviceToHost));
    MRX_HIP_TRY(hipMemcpy(spans, sp.p, sizeof(int32_t) * 2 * (size_t)tot, hipMemcpyDeviceToHost));
  }
  return rc;
}

void mrx_debug_kw_piece(int64_t bytes) { g_kw_piece.store(bytes > 0 ? bytes : 0); }
void mrx_debug_kw_tier(int on) { g_kw_lds.store(on ? 1 : 0); }

int mrx_debug_kw_host_findall(const uint8_t* entry_data, const int64_t* entry_offsets, int64_t m, uint32_t flags,
                              const uint8_t* data, const int64_t* offsets, int64_t n, int64_t* text_prefix, int32_t* entries,
                              int32_t* spans, int64_t span_cap, int64_t* total, char* describe, size_t describe_cap) {
  int dummy = 0;
  if (int rc = kw_check_build(m, flags, entry_offsets, &dummy)) return rc;
  if (n < 0 || span_cap < 0) return internal_fail(MRX_E_ARGUMENT, "n and span_cap must be >= 0");
  if (!offsets || !text_prefix || (span_cap > 0 && (!entries || !spans))) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (m > 0 && entry_offsets[m] > entry_offsets[0] && !entry_data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  const int64_t bytes = n > 0 ? offsets[n] - offsets[0] : 0;
  if (bytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  KwAutomaton A;
  if (int rc = kw_build_host(entry_data, entry_offsets, m, flags, &A)) return rc;
  (void)copy_text(kw_describe_text(A.m, A.distinct, A.states, A.ncls, A.lmax, A.flags), describe, describe_cap);
  // the texts at their own alignment inside a buffer that owns the aligned words around them
  const size_t skew = n > 0 ? (size_t)((uintptr_t)(data + offsets[0]) & 15) : 0;
  std::vector<g_u64x2> room((size_t)bytes / 16 + 3);
  uint8_t* copy = (uint8_t*)room.data() + skew;
  if (bytes > 0) memcpy(copy, data + offsets[0], (size_t)bytes);
  std::vector<int64_t> rel((size_t)n + 1, 0);
  for (int64_t i = 0; i <= n && n > 0; ++i) rel[(size_t)i] = offsets[i] - offsets[0];
  const int64_t pinned = g_kw_piece.load();
  const int64_t P = pinned > 0 ? pinned : kw_piece_rule(A.lmax, bytes);
  const int64_t tot = kw_host_findall(A, P, copy, rel.data(), n, text_prefix, entries, spans, span_cap);
  if (total) *total = tot;
  if (tot > span_cap) return internal_fail(MRX_E_CAPACITY, "span buffer too small: need " + std::to_string(tot));
  return MRX_OK;
}

}  // extern "C"
