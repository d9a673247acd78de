// captures_all on the device (gfx950 / CDNA4): the groups of every match of sub()'s loop.  The regex kernels
// underneath (findall, the literal prefilter, the prefix sums) are mrx_kernels.hip's, reached through mrx_core.hpp.
#include <string>

#include "mrx_core.hpp"
#include "mrx_chain_dev.hpp"

using namespace mrx;

// ---- captures_all: every match of sub()'s loop with a group template, and the groups that loop reads ----------------
// Three routes, chosen as sub_any() chooses them for a group template:
//   fixed-width groups on span-capable plans: findall's spans -> clamped counts -> k_scan_* -> k_capall_fixed;
//   deterministic chains: the plain search's spans -> k_capall_chain (the leaves' boundaries, as in k_subc_sizes);
//   everything else: sub_text()'s loop a lane per text, k_capall<CA_COUNT> -> k_scan_* -> k_capall<CA_EMIT>.
// A row is g + 1 int2: groups 1..g, then group 0; no row at or beyond match_cap is ever written.
namespace {
enum { CA_COUNT = 0, CA_EMIT = 1 };
// sub_text()'s loop without a byte sink: emit(k, ms, me, caps) for the k-th match; returns the number of matches.
// general: groups from NFAEngine.match_next_with_groups (caps), else the fixed-width form (caps unused).
template <int BT, class F>
__device__ inline int capall_text(const Ctx& c, const Text& t, bool general, long long count, F&& emit) {
  if (t.len == 0) return 0;
  int k = 0, pos = 0, ms, me;
  BtCaps caps;
  if constexpr (BT) if (general) {
    while (pos <= t.len) {
      if (!bt_match_next_with_groups<BT == 1>(c, t, pos, ms, me, caps)) break;
      if ((me == ms ? me + 1 : me) <= pos) break;   // a match in front of pos ends the list, as in sub_text()
      emit(k, ms, me, caps);
      ++k;
      pos = me == ms ? me + 1 : me;
      if (count > 0 && k >= count) break;
    }
    return k;
  }
  if (c.p.fixed_concat && t.len == c.p.fixed_total) {   // matcher.mojo:1726-1744: the whole text, if all digits
    for (int i = 0; i < c.p.fixed_total; ++i) {
      const int b = t.at(i);
      if (b < '0' || b > '9') return 0;
    }
    emit(0, 0, c.p.fixed_total, caps);
    return 1;
  }
  while (pos <= t.len) {
    if (!hybrid_match_next<BT>(c, t, pos, ms, me)) break;
    if ((me == ms ? me + 1 : me) <= pos) break;
    emit(k, ms, me, caps);
    ++k;
    pos = me == ms ? me + 1 : me;
    if (count > 0 && k >= count) break;
  }
  return k;
}
template <int MODE, int BT = 0>
__global__ __launch_bounds__(kBlock) void k_capall(DevPlan p, const uint8_t* __restrict__ blob, Layout lay, int64_t n,
                                                   int general, long long count, int32_t* __restrict__ counts,
                                                   const int64_t* __restrict__ prefix, int32_t* __restrict__ groups,
                                                   int64_t match_cap) {
  extern __shared__ __align__(16) uint8_t lds[];
  const Ctx c = stage_tables(p, blob, lds);
  const int g = general ? p.bt_ngroups : p.fixed_ngroups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const Text t = lay.text(i);
    if (MODE == CA_COUNT) {
      counts[i] = capall_text<BT>(c, t, general != 0, count, [](int, int, int, const BtCaps&) {});
    } else {
      const int64_t base = prefix[i];
      capall_text<BT>(c, t, general != 0, count, [&](int k, int ms, int me, const BtCaps& caps) {
        const int64_t row = base + k;
        if (row >= match_cap) return;
        int2* o = (int2*)(groups + row * (int64_t)(g + 1) * 2);
        for (int j = 1; j <= g; ++j)
          o[j - 1] = general ? make_int2(caps.gs(j), caps.ge(j))
                             : make_int2(ms + p.fixed_off[j], ms + p.fixed_off[j] + p.fixed_w[j]);
        o[g] = make_int2(ms, me);
      });
    }
  }
}
// matches kept per text: findall's, at most `count` (> 0), none in an empty text (sub_text() returns at once there)
__global__ __launch_bounds__(kBlock) void k_capall_clamp(int64_t n, const int64_t* __restrict__ offsets,
                                                         const int64_t* __restrict__ fprefix, long long count,
                                                         int32_t* __restrict__ counts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t k = offsets[i + 1] > offsets[i] ? fprefix[i + 1] - fprefix[i] : 0;
    if (count > 0 && k > count) k = count;
    counts[i] = (int32_t)k;
  }
}
// a wavefront per text; its lanes take the text's rows pair by pair, so the stores of a wavefront are one run
__global__ __launch_bounds__(kBlock) void k_capall_fixed(DevPlan p, int64_t n, const int64_t* __restrict__ fprefix,
                                                         const int32_t* __restrict__ spans, int64_t span_cap,
                                                         const int64_t* __restrict__ prefix, int32_t* __restrict__ groups,
                                                         int64_t match_cap) {
  if (fprefix[n] > span_cap) return;   // the spans are incomplete: the host repeats the findall
  const int g1 = p.fixed_ngroups + 1;
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); i < n; i += nw) {
    const int64_t a = prefix[i], sa = fprefix[i];
    int64_t kept = prefix[i + 1] - a;
    if (a + kept > match_cap) kept = match_cap > a ? match_cap - a : 0;
    const int64_t npairs = kept * g1;
    int2* o = (int2*)groups + a * g1;
    for (int64_t q = lane; q < npairs; q += 64) {
      const int64_t k = q / g1;
      const int j = (int)(q - k * g1);
      const int2 sp = *(const int2*)(spans + 2 * (sa + k));
      o[q] = j == g1 - 1 ? sp : make_int2(sp.x + p.fixed_off[j + 1], sp.x + p.fixed_off[j + 1] + p.fixed_w[j + 1]);
    }
  }
}
// the groups of a deterministic chain: a wavefront per text builds the leaves' bitmaps (subc_store), a lane per match
// finds the boundaries (subc_walk); group j lies between boundaries gb[j].x and gb[j].y
struct CapChainDev {
  ChainDev cd;
  int g;
  int2 gb[10];
};
template <int TILE>
__global__ __launch_bounds__(kBlock) void k_capall_chain(CapChainDev cc, int64_t n, const uint8_t* __restrict__ data,
                                                         const int64_t* __restrict__ offsets,
                                                         const int64_t* __restrict__ fprefix, const int32_t* __restrict__ spans,
                                                         int64_t span_cap, const uint8_t* __restrict__ g_mask,
                                                         const int64_t* __restrict__ prefix, int32_t* __restrict__ groups,
                                                         int64_t match_cap) {
  if (fprefix[n] > span_cap) return;
  constexpr int NB = TILE / 1024 + 1;
  constexpr int ROW = TILE / 16 + 4;
  __shared__ uint16_t bm_all[kBlock / 64][kSubcLeaves * ROW];
  __shared__ uint16_t bnd_all[kBlock / 64][64 * (kSubcLeaves + 1)];
  __shared__ uint8_t mask[256];
  for (int c = threadIdx.x; c < 256; c += blockDim.x) mask[c] = g_mask[c];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint16_t* bm = bm_all[wv];
  uint16_t* bnd = bnd_all[wv] + lane * (kSubcLeaves + 1);
  const int g1 = cc.g + 1;
  const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + wv; i < n; i += nw) {
    const int64_t a = prefix[i], sa = fprefix[i];
    int64_t kept = prefix[i + 1] - a;
    if (a + kept > match_cap) kept = match_cap > a ? match_cap - a : 0;
    const int64_t ibase = offsets[i];
    const int tlen = (int)(offsets[i + 1] - ibase);
    if (kept <= 0 || tlen > TILE) continue;   // (the host sends no text beyond the tile)
    const int k = (int)kept;
    const uint8_t* tptr = data + ibase;
    const int mis = (int)((uintptr_t)tptr & 15);
    const uint8_t* fptr = tptr - mis;
    const int nfb = (mis + tlen + 15) >> 4;
    uint4 tx[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      const int b = lane + 64 * r;
      tx[r] = b < nfb ? *(const uint4*)(fptr + 16 * b) : make_uint4(0, 0, 0, 0);
    }
    MRX_SUBC_WAVE_SYNC();   // (the previous text's walks are done with the bitmaps)
    subc_store<NB, ROW, false>(tx, bm, nullptr, mask, cc.cd.need, nfb, lane);
    MRX_SUBC_WAVE_SYNC();
    for (int m = lane; m < k; m += 64) {
      const int2 sp = *(const int2*)(spans + 2 * (sa + m));
      subc_walk<ROW>(cc.cd, bm, mis, bnd, sp.x, sp.y);
      int2* o = (int2*)groups + (a + m) * g1;
#pragma unroll
      for (int j = 1; j <= 9; ++j) {
        if (j > cc.g) break;
        o[j - 1] = make_int2((int)bnd[cc.gb[j].x], (int)bnd[cc.gb[j].y]);
      }
      o[cc.g] = sp;
    }
  }
}
}  // namespace

// captures_all's route for a CSR batch with no text beyond the chain kernel's tile (4096 bytes), from the plan alone:
// the rows of a deterministic chain from findall's spans (k_capall_chain), the fixed-width windows from findall's spans
// (k_capall_fixed), or sub_text()'s loop, a lane per text (k_capall_emit).  force_generic: mrx_debug_force_generic's level.
enum CapallRoute { CAPALL_GENERAL, CAPALL_FIXED, CAPALL_CHAIN };
static CapallRoute capall_route(const mrx_handle* h, int force_generic) {
  const HostPlan& hp = h->hp;
  const uint32_t sfl = hp.dev.flags;
  const bool general = hp.fixed_total < 0;
  const ChainGroups& cg = hp.chain;
  bool chain_ok = general && cg.ok && !force_generic && (sfl & (PF_STREAM_SEARCH | PF_STEP_SEARCH)) &&
                  hp.why_no_search.empty() && cg.nleaf <= kSubcLeaves && hp.bt.ngroups <= 9;
  for (int j = 1; chain_ok && j <= hp.bt.ngroups; ++j) chain_ok = cg.gopen[j] >= 0;
  if (chain_ok) return CAPALL_CHAIN;
  // (as sub_any's spans route: not with a memchr prefilter, not for exact literals, not for the whole-text shortcut of
  // "concat" patterns that are not purely groups)
  const bool spans_ok = !(sfl & PF_EXACT_LITERAL) &&
                        ((!force_generic && (sfl & PF_STREAM_SEARCH)) ||
                         (force_generic < 2 && (sfl & PF_STEP_SEARCH) && !(sfl & PF_PREFILTER)));
  const bool shortcut_differs = hp.fixed_concat && !hp.fixed_pure;
  if (spans_ok && !general && !shortcut_differs && hp.fixed_total < 0x7FFF) return CAPALL_FIXED;
  return CAPALL_GENERAL;
}
const char* mrx::capall_route_name(const mrx_handle* h) {
  const CapallRoute r = capall_route(h, 0);
  return r == CAPALL_CHAIN ? "chain" : r == CAPALL_FIXED ? "fixed" : "general";
}

static int capall_counts_to_prefix(const Layout& lay, int64_t n, const int64_t* d_fprefix, int64_t count,
                                   int32_t* d_counts, int64_t* d_prefix, int64_t* d_total, hipStream_t s) {
  hipLaunchKernelGGL(k_capall_clamp, dim3(device_grid(n, kBlock)), dim3(kBlock), 0, s, n, lay.offsets, d_fprefix,
                     (long long)count, d_counts);
  MRX_HIP_TRY(hipGetLastError());
  return device_scan<int32_t>(d_counts, n, d_prefix, d_total, s);
}

// routes 1 and 2: the spans of findall's match_next sequence, then the rows.  kSubsRetryGeneric: the batch is route 3's.
static int capall_from_spans(const mrx_handle* h, const Layout& lay, int64_t n, int64_t count, bool chain,
                             int64_t* d_prefix, int32_t* d_groups, int64_t match_cap, int64_t* total, hipStream_t s,
                             int64_t known_bytes, int64_t known_max) {
  int64_t in_bytes = known_bytes, max_len = known_max;
  if (known_bytes < 0 || known_max < 0)
    if (int rc0 = csr_stats(lay, n, s, &in_bytes, &max_len)) return rc0;
  if (in_bytes < 0) return internal_fail(MRX_E_ARGUMENT, "offsets[n] is negative");
  CapChainDev cc{};
  uint8_t mask8[256];
  if (chain) {
    const ChainGroups& cg = h->hp.chain;
    if (max_len > 4096) return kSubsRetryGeneric;   // (as sub_chain_from_spans: beyond the tile, the interpreter's)
    cc.cd.nleaf = cg.nleaf;
    for (int l = 0; l < kSubcLeaves; ++l) { cc.cd.lmax[l] = cg.lmax[l]; cc.cd.lfix[l] = l < cg.nleaf && cg.lmin[l] == cg.lmax[l] ? cg.lmin[l] : 0; }
    for (int l = 0; l + 1 < cg.nleaf; ++l) if (!cc.cd.lfix[l]) cc.cd.need |= 1 << l;
    cc.g = h->hp.bt.ngroups;
    for (int j = 1; j <= cc.g; ++j) cc.gb[j] = make_int2(cg.gopen[j], cg.gclose[j]);
    for (int c = 0; c < 256; ++c) mask8[c] = (uint8_t)cg.mask[c];
  }
  int64_t* d_fprefix = nullptr;
  int32_t *d_spans = nullptr, *d_counts = nullptr;
  int64_t* d_tot2 = nullptr;   // (kept rows, findall's spans: one copy to the host)
  uint8_t* d_mask = nullptr;
  MRX_SCRATCH(d_fprefix, sizeof(int64_t) * (n + 1), s);
  MRX_SCRATCH(d_counts, sizeof(int32_t) * n, s);
  MRX_SCRATCH(d_tot2, 2 * sizeof(int64_t), s);
  if (chain) {
    MRX_SCRATCH(d_mask, 256, s);
    MRX_HIP_TRY(hipMemcpyAsync(d_mask, mask8, 256, hipMemcpyHostToDevice, s));   // (pageable source: copied before the call returns)
  }
  int64_t cap = in_bytes / 8 + n + 64;
  if (const int64_t seen = h->sub_matches_per_kib.load(std::memory_order_relaxed); seen > 128) {
    const int64_t by_hint = (in_bytes >> 10) * (seen + seen / 8 + 1) + n + 64;
    if (by_hint > cap) cap = by_hint < in_bytes + n + 64 ? by_hint : in_bytes + n + 64;
  }
  int64_t h2[2] = {0, 0};
  const int64_t waves = (n + (kBlock / 64) - 1) / (kBlock / 64);
  const unsigned grid = (unsigned)(waves < grid_cap() ? waves : grid_cap());
  for (int attempt = 0; attempt < 2; ++attempt) {
    MRX_SCRATCH(d_spans, sizeof(int32_t) * 2 * (size_t)cap, s);
    if (int rc = run_findall(h, lay, n, d_fprefix, d_spans, cap, nullptr, s, /*match_next_sequence=*/true, in_bytes, max_len))
      return rc;
    if (int rc = capall_counts_to_prefix(lay, n, d_fprefix, count, d_counts, d_prefix, d_tot2, s)) return rc;
    // (the rows behind the spans without waiting: when the spans did not fit, the kernels return at once)
    if (!chain) {
      hipLaunchKernelGGL(k_capall_fixed, dim3(grid), dim3(kBlock), 0, s, h->hp.dev, n, d_fprefix, d_spans, cap, d_prefix,
                         d_groups, match_cap);
      set_last_kernel("k_capall_fixed");
    } else if (max_len <= 2048) {
      hipLaunchKernelGGL(k_capall_chain<2048>, dim3(grid), dim3(kBlock), 0, s, cc, n, lay.data, lay.offsets, d_fprefix,
                         d_spans, cap, d_mask, d_prefix, d_groups, match_cap);
      set_last_kernel("k_capall_chain");
    } else {
      hipLaunchKernelGGL(k_capall_chain<4096>, dim3(grid), dim3(kBlock), 0, s, cc, n, lay.data, lay.offsets, d_fprefix,
                         d_spans, cap, d_mask, d_prefix, d_groups, match_cap);
      set_last_kernel("k_capall_chain");
    }
    MRX_HIP_TRY(hipGetLastError());
    MRX_HIP_TRY(hipMemcpyAsync(d_tot2 + 1, d_fprefix + n, sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    MRX_HIP_TRY(hipMemcpyAsync(h2, d_tot2, sizeof h2, hipMemcpyDeviceToHost, s));
    MRX_HIP_TRY(hipStreamSynchronize(s));
    h->sub_matches_per_kib.store(in_bytes >= 1024 ? h2[1] / (in_bytes >> 10) : 0, std::memory_order_relaxed);
    if (h2[1] <= cap) break;
    if (attempt == 1) return internal_fail(MRX_E_NO_DEVICE, "captures_all: match count changed between two passes");
    cap = h2[1];   // more matches than the first guess: once more with room for all of them (behind the first attempt's)
  }
  *total = h2[0];
  if (h2[0] > match_cap) return internal_fail(MRX_E_CAPACITY, "group rows buffer too small: need " + std::to_string(h2[0]));
  return MRX_OK;
}

// (mrx_internal.hpp) what captures_all refuses, for the calls that put it in front of their own work (expand)
int mrx::captures_all_refusal(const mrx_handle* h) {
  // the groups sub() reads for a template such as "\\1": the general form unless the pattern has the fixed-width one
  if (h->hp.fixed_total < 0) {
    if (int rc = group_template_refusal(h)) return rc;
  } else if (int rc = check_search_supported(h)) {
    return rc;
  }
  return check_lds(h);
}

static int captures_all_any(const mrx_handle* h, int64_t count, const Layout& lay_in, int64_t n, int64_t* d_prefix,
                            int32_t* d_groups, int64_t match_cap, int64_t* total, void* st, int64_t known_bytes = -1,
                            int64_t known_max = -1) {
  ScratchScope scratch_scope_((hipStream_t)st);
  if (!h) return internal_fail(MRX_E_ARGUMENT, "null handle");
  if (!total) return internal_fail(MRX_E_ARGUMENT, "null total");
  *total = 0;
  if (n < 0) return internal_fail(MRX_E_ARGUMENT, "negative batch size");
  if (count < 0) return internal_fail(MRX_E_ARGUMENT, "negative count");
  if (match_cap < 0) return internal_fail(MRX_E_ARGUMENT, "negative match_cap");
  if (!d_prefix || (!d_groups && match_cap > 0)) return internal_fail(MRX_E_ARGUMENT, "null output buffer");
  if ((!lay_in.data && n > 0) || (!lay_in.offsets && lay_in.stride <= 0)) return internal_fail(MRX_E_ARGUMENT, "null batch");
  if (int rc = mrx::captures_all_refusal(h)) return rc;
  const bool general = h->hp.fixed_total < 0;
  if (int rc = ensure_device(h)) return rc;
  hipStream_t s = (hipStream_t)st;
  const int64_t* off = lay_in.offsets;
  const uint32_t sfl = h->hp.dev.flags;
  // (the spans routes take CSR batches; a chain batch with a text beyond the tile comes back for route 3)
  const CapallRoute route = n > 0 && off ? capall_route(h, force_generic()) : CAPALL_GENERAL;
  if (route == CAPALL_CHAIN) {
    const int rc = capall_from_spans(h, csr(lay_in.data, off), n, count, true, d_prefix, d_groups,
                                     match_cap, total, s, known_bytes, known_max);
    if (rc != kSubsRetryGeneric) return rc;
  }
  if (route == CAPALL_FIXED)
    return capall_from_spans(h, csr(lay_in.data, off), n, count, false, d_prefix, d_groups, match_cap,
                             total, s, known_bytes, known_max);
  // route 3: sub_text()'s loop, a lane per text
  Layout lay = lay_in;
  if ((sfl & PF_BT_SEARCH) || general) {
    const Layout plain = lay;
    if (int rc = bt_prepass(h, plain, n, s, &lay)) return rc;
  }
  const bool use_bt = plan_uses_backtracker(h) || general;
  int32_t* d_counts = nullptr;
  int64_t* d_total = nullptr;
  MRX_SCRATCH(d_counts, sizeof(int32_t) * (n > 0 ? n : 1), s);
  MRX_SCRATCH(d_total, sizeof(int64_t), s);
  if (n > 0) {
    ScanTimer tm(s);
#define MRX_L(B) hipLaunchKernelGGL((k_capall<CA_COUNT, B>), dim3(device_grid(n, kBlock)), dim3(kBlock), lds_for(h), s, h->hp.dev, \
                                   H_BLOB(h), lay, n, general ? 1 : 0, (long long)count, d_counts, (const int64_t*)nullptr,    \
                                   (int32_t*)nullptr, (int64_t)0)
    MRX_BT_DISPATCH(bt_kernel_kind(h, use_bt), MRX_L);
#undef MRX_L
    set_last_kernel("k_capall_count");
    MRX_HIP_TRY(hipGetLastError());
    tm.stop();
  }
  if (int rc = device_scan<int32_t>(d_counts, n, d_prefix, d_total, s)) return rc;
  if (n > 0 && match_cap > 0) {   // (enqueued before the total is known: rows at or beyond match_cap are not written)
#define MRX_L(B) hipLaunchKernelGGL((k_capall<CA_EMIT, B>), dim3(device_grid(n, kBlock)), dim3(kBlock), lds_for(h), s, h->hp.dev, \
                                   H_BLOB(h), lay, n, general ? 1 : 0, (long long)count, (int32_t*)nullptr, d_prefix,        \
                                   d_groups, match_cap)
    MRX_BT_DISPATCH(bt_kernel_kind(h, use_bt), MRX_L);
#undef MRX_L
    set_last_kernel("k_capall_emit");
    MRX_HIP_TRY(hipGetLastError());
  }
  int64_t tot = 0;
  MRX_HIP_TRY(hipMemcpyAsync(&tot, d_total, sizeof tot, hipMemcpyDeviceToHost, s));
  MRX_HIP_TRY(hipStreamSynchronize(s));
  *total = tot;
  if (tot > match_cap) return internal_fail(MRX_E_CAPACITY, "group rows buffer too small: need " + std::to_string(tot));
  return MRX_OK;
}

extern "C" {
int mrx_captures_all_dev(const mrx_handle* h, const uint8_t* d, const int64_t* off, int64_t n, int64_t count,
                         int64_t* d_match_prefix, int32_t* d_groups, int64_t match_cap, int64_t* total, void* st) {
  const TextBatch b = csr(d, off);
  if (int rc = check_batch(b, BATCH_CSR)) return rc;
  return captures_all_any(h, count, b, n, d_match_prefix, d_groups, match_cap, total, st);
}
// Texts at a fixed pitch, as mrx_sub_strided_dev: rows without padding are a CSR batch (offsets i * stride written on the
// device) and take every route; padded rows take the lane-per-text kernels.
int mrx_captures_all_strided_dev(const mrx_handle* h, const uint8_t* d, int64_t stride, const int32_t* d_lens, int32_t len,
                                 int64_t n, int64_t count, int64_t* d_match_prefix, int32_t* d_groups, int64_t match_cap,
                                 int64_t* total, void* st) {
  const TextBatch b = strided(d, stride, d_lens, len);
  if (int rc = check_batch(b, BATCH_PITCH_TERSE)) return rc;
  if (h && total && count >= 0 && rows_unpadded(b, n)) {
    ScratchScope scope_((hipStream_t)st);
    TextBatch rows;
    if (int rc = rows_as_csr(b, n, st, &rows)) return rc;
    return captures_all_any(h, count, rows, n, d_match_prefix, d_groups, match_cap, total, st, n * stride, stride);
  }
  return captures_all_any(h, count, b, n, d_match_prefix, d_groups, match_cap,
                          total, st);
}
int mrx_captures_all_batch(const mrx_handle* h, const uint8_t* data, const int64_t* off, int64_t n, int64_t count,
                           int64_t* match_prefix, int32_t* groups, int64_t match_cap, int64_t* total) {
  if (!h || !total || !match_prefix || (!groups && match_cap > 0)) return internal_fail(MRX_E_ARGUMENT, "null argument");
  if (match_cap < 0) return internal_fail(MRX_E_ARGUMENT, "negative match_cap");
  DevBatch b; DevBuf<int64_t> pre; DevBuf<int32_t> gr;
  if (int rc = b.upload(data, off, n)) return rc;
  if (int rc = pre.alloc(n + 1)) return rc;
  const size_t per = (size_t)(mrx_num_groups(h) + 1) * 2;
  if (int rc = gr.alloc(per * (size_t)match_cap)) return rc;
  int64_t tot = 0;
  const int rc = mrx_captures_all_dev(h, b.data, b.offsets, n, count, pre.p, gr.p, match_cap, &tot, nullptr);
  *total = tot;
  if (rc != MRX_OK && rc != MRX_E_CAPACITY) return rc;
  MRX_HIP_TRY(hipMemcpy(match_prefix, pre.p, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost));
  if (rc == MRX_OK && tot > 0) MRX_HIP_TRY(hipMemcpy(groups, gr.p, sizeof(int32_t) * per * (size_t)tot, hipMemcpyDeviceToHost));
  return rc;
}
}  // extern "C"
