// Keywords: what mrx_keywords.hip (contains, count, findall, filter) and mrx_kw_sub.hip (leftmost, sub) share -- the
// handle, the view of an automaton that a walk reads, the LDS tier and the piece of a lane.  Device code of the two
// translation units only; the automaton and the walks themselves are in mrx_kw_bits.hpp and mrx_kw_sub_bits.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mrx.h"
#include "mrx_internal.hpp"
#include "mrx_kw_bits.hpp"

// one automaton in device memory that the handle owns
struct mrx_kw_tables {
  int32_t states = 1, ncls = 1;
  uint32_t* table = nullptr;    // [states * ncls]
  uint8_t* cls = nullptr;       // [256]
  mrx::KwMeta* meta = nullptr;  // [states]
  ~mrx_kw_tables() {
    if (table) (void)hipFree(table);
    if (cls) (void)hipFree(cls);
    if (meta) (void)hipFree(meta);
  }
};

// Immutable for its callers once mrx_kw_build* has returned.  The automaton over the REVERSED entries, which only
// leftmost and sub walk, is built from the host copy of the folded entries at the first such call, under rev_once: its
// outcome (rev_rc, rev_err) is remembered, and a refusal leaves every other operation as it was.
struct mrx_kw {
  int64_t m = 0, distinct = 0;
  int32_t lmax = 0;
  uint32_t flags = 0;
  mrx_kw_tables fwd;
  std::vector<uint8_t> entry_data;    // the folded entries, packed
  std::vector<int64_t> entry_off;     // [m + 1]
  mutable std::once_flag rev_once;
  mutable mrx_kw_tables rev;
  mutable int rev_rc = 0;
  mutable std::string rev_err;
};

namespace mrx {

constexpr int kKwBlock = 512;
constexpr int kKwTierWords = 8192;   // 32 KiB of table rows in LDS: four workgroups, 2048 lanes, a CU
constexpr unsigned kKwMaxGrid = 1024;

// what a walk reads of the handle
struct KwView {
  const uint32_t* table;
  const uint8_t* cls;
  const KwMeta* meta;
  int32_t ncls, lmax;
  uint32_t tier;   // states whose rows the workgroups keep in LDS
};

// mrx_keywords.hip: the hooks' state, the view of one of the handle's automata under them, and the pieces of a call on
// a checked batch of n >= 1 texts inside the caller's ScratchScope (known_total / known_max: a CSR batch's bounds, < 0:
// read back, one synchronisation)
int64_t kw_pinned_piece();
KwView kw_view(const mrx_kw_tables& t, int32_t lmax);
int kw_plan_pieces(int32_t lmax, const TextBatch& b, int64_t n, int64_t known_total, int64_t known_max, KwPieces& pc, void* st);
// the build's checks and the build with the caller's error text, and one automaton's upload (enqueued on `stream`)
int kw_check_build(int64_t m, uint32_t flags, const void* offsets, const void* out);
int kw_build_host(const uint8_t* data, const int64_t* offsets, int64_t m, uint32_t flags, KwAutomaton* A);
int kw_upload_tables(const KwAutomaton& A, void* stream, mrx_kw_tables* t);

#if defined(__HIPCC__)
namespace {
// (at file scope, so that the walk's loads from them are LDS loads by their type, not loads through a generic pointer)
__shared__ uint32_t s_kw_tab[kKwTierWords];
__shared__ uint8_t s_kw_cls[256];

struct KwDevTab {
  const uint32_t* __restrict__ g;
  int32_t ncls;
  uint32_t tier;
  __device__ __forceinline__ uint32_t word(uint32_t st, uint32_t byte) const {
    // (the global pointer carries its address space: through a generic one the compiler merges the two loads into
    // one flat load whose address is chosen per lane)
    typedef const __attribute__((address_space(1))) uint32_t* GlobalWords;
    const uint32_t i = st * (uint32_t)ncls + s_kw_cls[byte];
    if (st < tier) return s_kw_tab[i];
    return ((GlobalWords)g)[i];
  }
};

// every workgroup of a walking kernel, first: the tier's rows and the class map into LDS
__device__ __forceinline__ KwDevTab kw_stage_tier(const KwView& V) {
  const uint32_t tier_words = V.tier * (uint32_t)V.ncls;
  for (uint32_t k = threadIdx.x; k < tier_words; k += kKwBlock) s_kw_tab[k] = V.table[k];
  if (threadIdx.x < 256) s_kw_cls[threadIdx.x] = V.cls[threadIdx.x];
  __syncthreads();
  return KwDevTab{V.table, V.ncls, V.tier};
}
}  // namespace
#endif

}  // namespace mrx
