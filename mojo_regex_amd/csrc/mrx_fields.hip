// Fields (include/mrx.h, "fields"): the delimiter- or whitespace-separated columns of every text as one fixed-width row
// of (start, end) pairs.  One kernel, k_fields; no scratch, no atomics, no inline assembly, nothing read back, and no
// wavefront waits for another.
//
// Route.  A group of G lanes takes a text, G a power of two from 1 to 64, so a wavefront takes 64 / G
// neighbouring texts a round and a contiguous run of texts over its rounds, as k_parse takes its rows.  Each round of a
// walk, lane l of a group loads aligned 16-byte word w0 + l of its text, masks the bytes outside the text and turns the
// word into its event masks (mrx_fields_bits.hpp).  A prefix sum of the popcounts over the group's lanes (log2 G
// shuffles, both event kinds in one word) ranks every event within the text; the lane whose word holds a wanted rank
// writes the position into the row, which is staged in LDS: (64 / G) x f pairs per wavefront.  The walk is uniform over
// the wavefront (a group whose text has ended idles with empty masks), so every shuffle runs with all lanes active.
// Negative columns need nf: they take a second walk over the text, by then in cache, with their ranks resolved.
// Behind the walks the wavefront's rows, which are neighbours in the output, leave as whole 8-byte pairs, lane after
// lane: one coalesced run of (64 / G) x f x 8 bytes.
//
// G is chosen per call from the mean text length where the call knows it (fields_group_rule, from the sweep of
// profiles/fields.md: 1, 2 or 4 lanes for texts of up to 16 KiB); a text takes as many rounds of 16 G bytes as it is
// long.  One text of many MiB is answered by a single group: right, not fast.
//
// Quoted fields (mrx_fields_quoted_*) are the same kernel with QUOTED = true: the quote bits of the word a lane holds,
// their prefix-xor, one ballot a round for the parity of the lanes in front within the group and one carried bit make
// the inside mask; the outer quotes of a pair are decided where the pairs leave the stage.  The instances with
// QUOTED = false are the code they were.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "../../include/mrx_testing.h"
#include "mrx_fields_bits.hpp"
#include "mrx_host_batch.hpp"
#include "mrx_internal.hpp"

namespace mrx {
namespace {

constexpr int kFieldsBlock = 256;
constexpr unsigned kFieldsMaxGrid = 2048;   // 8 workgroups per CU, as k_parse; a wavefront strides over what is left
constexpr size_t kFieldsMaxLds = 32768;     // of row staging per workgroup: more than this and the workgroup shrinks

std::atomic<int> g_fields_group{0};   // mrx_debug_fields_group(): the pinned G (0 = the rule)
std::atomic<int> g_fields_grid{0};    // mrx_debug_fields_grid(): workgroups at most (0 = no cap of its own)
std::atomic<int> g_fields_last_group{0};   // mrx_debug_fields_last_group(): the G of the last launch (0 = none yet)

struct FieldsOut {
  int32_t* rows;
  int32_t* nf;
  int64_t* prefix;
};
// quoted fields: the quote byte and the quoted bytes uint8[n][f] (may be null).  The last kernel argument, so that the
// arguments in front of it lie where they lay; the instances without quotes never read it
struct FieldsQuote {
  uint8_t* quoted;
  uint32_t quote;
};

// LDS writes of one lane are read by another lane of the same wavefront behind this
__device__ __forceinline__ void fields_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G, bool QUOTED>
__global__ __launch_bounds__(kFieldsBlock) void k_fields(const TextBatch B, int64_t n, const FieldsPlan P, const FieldsOut O,
                                                         const FieldsQuote Q) {
  extern __shared__ __align__(8) int32_t fields_lds[];
  constexpr int T = 64 / G;   // texts of a wavefront's round
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int gl = lane & (G - 1), t = lane / G;
  int32_t* tile = fields_lds + wave * (T * P.f * 2);
  int32_t* row = tile + t * P.f * 2;
  const int64_t nw = (int64_t)gridDim.x * ((int)blockDim.x >> 6), w = (int64_t)blockIdx.x * ((int)blockDim.x >> 6) + wave;
  // a wavefront takes a contiguous run of texts, T a round
  const int64_t per = ((n + nw - 1) / nw + (T - 1)) & ~(int64_t)(T - 1);
  const int64_t t_begin = w * per, t_end = t_begin + per < n ? t_begin + per : n;
  const bool ws = fields_ws_mode(P);
  for (int64_t i0 = t_begin; i0 < t_end; i0 += T) {
    const int64_t i = i0 + t;
    const bool live = i < t_end;
    int32_t L = 0;
    const uint8_t* tp = B.data;
    if (live) {
      tp = B.text(i, &L);
      if (L < 0) L = 0;
    }
    const int head = (int)((uintptr_t)tp & 15);
    const uint8_t* base = tp - head;
    const int64_t nwords = live ? fields_words(head, L) : 0;
    int32_t nf = 0;
    for (int pass = 0; pass < (P.any_neg ? 2 : 1); ++pass) {
      const bool negative = pass == 1;
      fields_wave_sync();   // the row's last readers are done with it
      fields_row_init(P, negative, nf, L, row, gl, G);
      fields_wave_sync();
      int64_t ra = 0, rb = 0;   // the events of the text in front of the round
      uint32_t carry = 0;
      uint32_t parity = 0;   // QUOTED: the quotes of the text in front of the round are odd; every walk begins outside
      bool done = false;
      for (int64_t w0 = 0;; w0 += G) {
        if (!negative && P.stop && fields_done(P, ra, rb)) done = true;
        const bool more = !done && w0 < nwords;
        if (!__any(more)) break;
        const int64_t wi = w0 + gl;
        uint32_t m = 0;
        if constexpr (QUOTED) {
          g_u128 word = 0;
          uint32_t valid = 0;
          if (more && wi < nwords) {
            word = gather_window(base + 16 * wi, 16);
            valid = fields_valid(head, L, wi);
          }
          const uint32_t q = lines_eq16(word, Q.quote) & valid;
          // one ballot: the lanes whose word holds an odd number of quotes.  The walk is uniform, all lanes are here
          const uint64_t mine = fields_group_bits(__ballot(lines_popc(q) & 1), t, G);
          m = fields_word_mask_quoted(P, word, valid, fields_inside(q, fields_parity_front(mine, gl) ^ parity));
          parity ^= fields_parity_all(mine);
        } else {
          if (more && wi < nwords) m = fields_word_mask(P, gather_window(base + 16 * wi, 16), fields_valid(head, L, wi));
        }
        uint32_t a = m, b = m;
        if (ws) {
          const uint32_t up = (uint32_t)__shfl_up((int)m, 1, G);
          const uint32_t cin = gl == 0 ? carry : (up >> 15) & 1u;
          carry = ((uint32_t)__shfl((int)m, G - 1, G) >> 15) & 1u;
          a = fields_starts(m, cin);
          b = fields_ends(m, cin);
        }
        // both counts in one word: at most 16 x 64 of either in a round
        const uint32_t mine = (uint32_t)lines_popc(a) | ((uint32_t)lines_popc(b) << 16);
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < G; d <<= 1) {
          const uint32_t v = (uint32_t)__shfl_up((int)incl, d, G);
          if (gl >= d) incl += v;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, G - 1, G), excl = incl - mine;
        if (a | b) fields_select(P, negative, nf, a, b, ra + (excl & 0xffffu), rb + (excl >> 16), 16 * wi - head, row);
        ra += total & 0xffffu;
        rb += total >> 16;
      }
      if (!negative) nf = fields_count(P, ra);
    }
    fields_wave_sync();
    // the round's rows are neighbours in the output: whole pairs, lane after lane
    const int64_t texts = t_end - i0 < T ? t_end - i0 : T;
    const int pairs = (int)texts * P.f;
    int32_t* out = O.rows + 2 * (i0 * P.f);
    if constexpr (QUOTED) {
      // the outer quotes are decided here: the lane that stores pair p reads t[s] and t[e - 1] of that pair's text,
      // whose address the first lane of its group holds.  Uniform trips, so that every source lane is there
      const uint32_t tp_lo = (uint32_t)(uintptr_t)tp, tp_hi = (uint32_t)((uintptr_t)tp >> 32);
      for (int p0 = 0; p0 < pairs; p0 += 64) {
        const int p = p0 + lane;
        const int src = (p < pairs ? p / P.f : 0) * G;
        const uint32_t lo = (uint32_t)__shfl((int)tp_lo, src), hi = (uint32_t)__shfl((int)tp_hi, src);
        if (p < pairs) {
          int2 v = *(const int2*)(tile + 2 * p);
          fields_finish(&v.x, &v.y);
          const uint8_t was = fields_unquote((const uint8_t*)(((uintptr_t)hi << 32) | lo), Q.quote, &v.x, &v.y);
          *(int2*)(out + 2 * p) = v;
          if (Q.quoted) Q.quoted[i0 * P.f + p] = was;
        }
      }
    } else {
      for (int p = lane; p < pairs; p += 64) {
        int2 v = *(const int2*)(tile + 2 * p);
        fields_finish(&v.x, &v.y);
        *(int2*)(out + 2 * p) = v;
      }
    }
    if (live && gl == 0) {
      if (O.nf) O.nf[i] = nf;
      if (O.prefix) {
        O.prefix[i] = i;
        if (i == n - 1) O.prefix[n] = n;
      }
    }
  }
}

int pinned_or(int rule) {
  const int g = g_fields_group.load(std::memory_order_relaxed);
  return g > 0 ? g : rule;
}

int launch(const TextBatch& b, int64_t n, const FieldsPlan& p, int g, const FieldsOut& o, int quote, uint8_t* d_quoted, void* stream) {
  const int texts_per_wave = 64 / g;
  int block = kFieldsBlock;
  const size_t per_wave = (size_t)texts_per_wave * (size_t)p.f * 8;
  while (block > 64 && per_wave * (size_t)(block / 64) > kFieldsMaxLds) block >>= 1;
  const size_t lds = per_wave * (size_t)(block / 64);
  const unsigned grid = grid_for(n, (int64_t)texts_per_wave * (block / 64), kFieldsMaxGrid, g_fields_grid.load(std::memory_order_relaxed));
  hipStream_t hs = (hipStream_t)stream;
  const FieldsQuote q{d_quoted, quote >= 0 ? (uint32_t)quote : 0u};
  switch (g) {
#define MRX_FIELDS_CASE(GG)                                                                                     \
  case GG:                                                                                                      \
    if (quote >= 0) hipLaunchKernelGGL((k_fields<GG, true>), dim3(grid), dim3(block), lds, hs, b, n, p, o, q);  \
    else hipLaunchKernelGGL((k_fields<GG, false>), dim3(grid), dim3(block), lds, hs, b, n, p, o, q);            \
    break;
    MRX_FIELDS_CASE(1) MRX_FIELDS_CASE(2) MRX_FIELDS_CASE(4) MRX_FIELDS_CASE(8) MRX_FIELDS_CASE(16) MRX_FIELDS_CASE(32)
    MRX_FIELDS_CASE(64)
#undef MRX_FIELDS_CASE
    default: return internal_fail(MRX_E_ARGUMENT, "bad group");
  }
  MRX_HIP_TRY(hipGetLastError());
  set_last_kernel("k_fields");
  g_fields_last_group.store(g, std::memory_order_relaxed);
  return MRX_OK;
}

struct FieldsCall {
  uint32_t flags;
  uint8_t delim;
  const int32_t* columns;
  int32_t f;
  int32_t* d_rows;
  int32_t* d_nf;
  int64_t* d_prefix;
  void* stream;
  int quote = -1;   // >= 0: quoted fields with that quote byte
  uint8_t* d_quoted = nullptr;
};

// argument errors: nothing has touched the device when one of them returns.  mean_len < 0: not known
int fields_run(const TextBatch& b, BatchForm form, int64_t n, int64_t mean_len, const FieldsCall& c) {
  FieldsPlan p;
  if (const char* msg = fields_plan(c.flags, c.delim, c.columns, c.f, c.d_nf != nullptr, &p)) return internal_fail(MRX_E_ARGUMENT, msg);
  if (c.quote >= 0)
    if (const char* msg = fields_quote_check(c.flags, c.delim, (uint8_t)c.quote)) return internal_fail(MRX_E_ARGUMENT, msg);
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (int rc = check_batch(b, form)) return rc;
  if (!c.d_rows) return internal_fail(MRX_E_ARGUMENT, c.d_quoted ? "d_quoted needs d_rows" : "null argument");
  if ((uintptr_t)c.d_rows & 7) return internal_fail(MRX_E_ARGUMENT, "d_rows must be 8-byte aligned");
  if (n == 0) return MRX_OK;
  return launch(b, n, p, pinned_or(fields_group_rule(mean_len)), FieldsOut{c.d_rows, c.d_nf, c.d_prefix}, c.quote, c.d_quoted, c.stream);
}

// mrx_fields_batch and mrx_fields_quoted_batch (quote >= 0; quoted may be null)
int fields_batch(uint32_t flags, uint8_t delim, int quote, const int32_t* columns, int32_t f, const uint8_t* data, const int64_t* offsets,
                 int64_t n, int32_t* rows, int32_t* nf, uint8_t* quoted, int64_t* prefix) {
  FieldsPlan p;
  if (const char* msg = fields_plan(flags, delim, columns, f, nf != nullptr, &p)) return internal_fail(MRX_E_ARGUMENT, msg);
  if (quote >= 0)
    if (const char* msg = fields_quote_check(flags, delim, (uint8_t)quote)) return internal_fail(MRX_E_ARGUMENT, msg);
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (quoted && !rows) return internal_fail(MRX_E_ARGUMENT, "d_quoted needs d_rows");
  if (!offsets || !rows) return internal_fail(MRX_E_ARGUMENT, "null argument");
  DevBatch b; DevBuf<int32_t> dr, dn; DevBuf<int64_t> dp; DevBuf<uint8_t> dq;
  if (int rc = b.measure(offsets, n)) return rc;
  if (b.nbytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (b.nbytes > 0 && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (n == 0) return MRX_OK;
  if (int rc = b.upload(data, offsets, n)) return rc;
  if (int rc = dr.alloc((size_t)n * (size_t)f * 2)) return rc;
  if (nf) if (int rc = dn.alloc((size_t)n)) return rc;
  if (prefix) if (int rc = dp.alloc((size_t)n + 1)) return rc;
  if (quoted) if (int rc = dq.alloc((size_t)n * (size_t)f)) return rc;
  FieldsCall c{flags, delim, columns, f, dr.p, nf ? dn.p : nullptr, prefix ? dp.p : nullptr, nullptr};
  c.quote = quote;
  c.d_quoted = quoted ? dq.p : nullptr;
  if (int rc = fields_run(csr(b.data, b.offsets), BATCH_CSR, n, b.nbytes / n, c)) return rc;
  MRX_HIP_TRY(hipMemcpy(rows, dr.p, sizeof(int32_t) * (size_t)n * (size_t)f * 2, hipMemcpyDeviceToHost));
  if (nf) MRX_HIP_TRY(hipMemcpy(nf, dn.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (quoted) MRX_HIP_TRY(hipMemcpy(quoted, dq.p, (size_t)n * (size_t)f, hipMemcpyDeviceToHost));
  if (prefix) MRX_HIP_TRY(hipMemcpy(prefix, dp.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost));
  return MRX_OK;
}

// mrx_debug_fields_host and mrx_debug_fields_quoted_host (quote >= 0; quoted may be null)
int fields_host(uint32_t flags, uint8_t delim, int quote, const int32_t* columns, int32_t f, const uint8_t* data, const int64_t* offsets,
                int64_t n, int32_t* rows, int32_t* nf, uint8_t* quoted, int64_t* prefix) {
  FieldsPlan p;
  if (const char* msg = fields_plan(flags, delim, columns, f, nf != nullptr, &p)) return internal_fail(MRX_E_ARGUMENT, msg);
  if (quote >= 0)
    if (const char* msg = fields_quote_check(flags, delim, (uint8_t)quote)) return internal_fail(MRX_E_ARGUMENT, msg);
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "n must be >= 0");
  if (quoted && !rows) return internal_fail(MRX_E_ARGUMENT, "d_quoted needs d_rows");
  if (!offsets || !rows) return internal_fail(MRX_E_ARGUMENT, "null argument");
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return internal_fail(MRX_E_ARGUMENT, "offsets must not decrease");
  if (n == 0) return MRX_OK;
  if (offsets[n] > offsets[0] && !data) return internal_fail(MRX_E_ARGUMENT, "null argument");
  const int g = pinned_or(fields_group_rule((offsets[n] - offsets[0]) / n));
  // the texts in a buffer of its own, at their alignment, with whole words around them: the walk loads aligned words
  const int64_t lo = offsets[0], nbytes = offsets[n] - lo;
  const int skew = (int)((uintptr_t)(data + lo) & 15);
  std::vector<uint8_t> store((size_t)nbytes + 48);
  for (size_t k = 0; k < store.size(); ++k) store[k] = k % 3 == 0 ? delim : k % 3 == 1 ? (uint8_t)' ' : (uint8_t)'q';
  if (quote >= 0)   // quote bytes around the texts too: an odd number in front of the first one
    for (size_t k = 0; k < store.size(); k += 2) store[k] = (uint8_t)quote;
  uint8_t* at = store.data() + ((16 - ((uintptr_t)store.data() & 15)) & 15) + skew;
  for (int64_t k = 0; k < nbytes; ++k) at[k] = data[lo + k];
  for (int64_t i = 0; i < n; ++i) {
    int32_t one = 0;
    fields_host_text(p, g, at + (offsets[i] - lo), offsets[i + 1] - offsets[i], rows + 2 * i * f, &one, quote, quoted ? quoted + i * f : nullptr);
    if (nf) nf[i] = one;
    if (prefix) prefix[i] = i;
  }
  if (prefix) prefix[n] = n;
  return MRX_OK;
}

}  // namespace
}  // namespace mrx

using namespace mrx;

extern "C" {

int mrx_fields_dev(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* d_data,
                   const int64_t* d_offsets, int64_t n, int32_t* d_rows, int32_t* d_nf, int64_t* d_prefix, void* stream) {
  return fields_run(csr(d_data, d_offsets), BATCH_CSR, n, -1, FieldsCall{flags, delim, columns, f, d_rows, d_nf, d_prefix, stream});
}
int mrx_fields_known_dev(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* d_data,
                         const int64_t* d_offsets, int64_t n, int64_t end_offset, int64_t max_text_len, int32_t* d_rows,
                         int32_t* d_nf, int64_t* d_prefix, void* stream) {
  if (end_offset < 0 || max_text_len < 0) return internal_fail(MRX_E_ARGUMENT, "end_offset and max_text_len must be >= 0");
  return fields_run(csr(d_data, d_offsets), BATCH_CSR, n, n > 0 ? end_offset / n : -1,
                    FieldsCall{flags, delim, columns, f, d_rows, d_nf, d_prefix, stream});
}
int mrx_fields_strided_dev(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* d_data,
                           int64_t stride, const int32_t* d_lens, int32_t len, int64_t n, int32_t* d_rows, int32_t* d_nf,
                           int64_t* d_prefix, void* stream) {
  return fields_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n, d_lens ? stride : (int64_t)len,
                    FieldsCall{flags, delim, columns, f, d_rows, d_nf, d_prefix, stream});
}

static FieldsCall quoted_call(uint32_t flags, uint8_t delim, uint8_t quote, const int32_t* columns, int32_t f, int32_t* d_rows,
                              int32_t* d_nf, uint8_t* d_quoted, int64_t* d_prefix, void* stream) {
  FieldsCall c{flags, delim, columns, f, d_rows, d_nf, d_prefix, stream};
  c.quote = quote;
  c.d_quoted = d_quoted;
  return c;
}
int mrx_fields_quoted_dev(uint32_t flags, uint8_t delim, uint8_t quote, const int32_t* columns, int32_t f, const uint8_t* d_data,
                          const int64_t* d_offsets, int64_t n, int32_t* d_rows, int32_t* d_nf, uint8_t* d_quoted,
                          int64_t* d_prefix, void* stream) {
  return fields_run(csr(d_data, d_offsets), BATCH_CSR, n, -1,
                    quoted_call(flags, delim, quote, columns, f, d_rows, d_nf, d_quoted, d_prefix, stream));
}
int mrx_fields_quoted_strided_dev(uint32_t flags, uint8_t delim, uint8_t quote, const int32_t* columns, int32_t f,
                                  const uint8_t* d_data, int64_t stride, const int32_t* d_lens, int32_t len, int64_t n,
                                  int32_t* d_rows, int32_t* d_nf, uint8_t* d_quoted, int64_t* d_prefix, void* stream) {
  return fields_run(strided(d_data, stride, d_lens, len), BATCH_PITCH, n, d_lens ? stride : (int64_t)len,
                    quoted_call(flags, delim, quote, columns, f, d_rows, d_nf, d_quoted, d_prefix, stream));
}

int mrx_fields_batch(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* data,
                     const int64_t* offsets, int64_t n, int32_t* rows, int32_t* nf, int64_t* prefix) {
  return fields_batch(flags, delim, -1, columns, f, data, offsets, n, rows, nf, nullptr, prefix);
}
int mrx_fields_quoted_batch(uint32_t flags, uint8_t delim, uint8_t quote, const int32_t* columns, int32_t f, const uint8_t* data,
                            const int64_t* offsets, int64_t n, int32_t* rows, int32_t* nf, uint8_t* quoted, int64_t* prefix) {
  return fields_batch(flags, delim, quote, columns, f, data, offsets, n, rows, nf, quoted, prefix);
}

int mrx_debug_fields_group(int lanes) {
  if (lanes == 0) g_fields_group = 0;
  else if (lanes >= 1 && lanes <= 64 && (lanes & (lanes - 1)) == 0) g_fields_group = lanes;
  return g_fields_group.load();
}
void mrx_debug_fields_grid(int workgroups) { g_fields_grid = workgroups > 0 ? workgroups : 0; }
int mrx_debug_fields_last_group(void) { return g_fields_last_group.load(); }

int mrx_debug_fields_host(uint32_t flags, uint8_t delim, const int32_t* columns, int32_t f, const uint8_t* data,
                          const int64_t* offsets, int64_t n, int32_t* rows, int32_t* nf, int64_t* prefix) {
  return fields_host(flags, delim, -1, columns, f, data, offsets, n, rows, nf, nullptr, prefix);
}
int mrx_debug_fields_quoted_host(uint32_t flags, uint8_t delim, uint8_t quote, const int32_t* columns, int32_t f,
                                 const uint8_t* data, const int64_t* offsets, int64_t n, int32_t* rows, int32_t* nf,
                                 uint8_t* quoted, int64_t* prefix) {
  return fields_host(flags, delim, quote, columns, f, data, offsets, n, rows, nf, quoted, prefix);
}

}  // extern "C"
