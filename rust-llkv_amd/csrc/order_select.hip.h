// order_select.hip.h — what the exact radix selects over composite order keys share (group_order.hip: the groups of a GROUP BY,
// scan_topn.hip: the selected rows of a projection scan): the bounds, the threshold state, the order-preserving images.
#pragma once

#include "engine.hpp"

#include <algorithm>

namespace llkv {

namespace {

constexpr int kMaxTerms = 8;
constexpr int kMaxWords = 16;   // order-key words of the terms (a term: its NULL word and one or two value words)
constexpr uint32_t kOrderBlock = 256;

// Threshold of the radix select: the composite keys (words 0 … n_words − 1, then the position) whose bits under `mask` equal
// `prefix` are still tied with it; `need` of them are still to be taken.
struct SelectState {
  unsigned long long need;
  uint32_t done, pad;
  unsigned long long prefix[kMaxWords + 1], mask[kMaxWords + 1];
};

__device__ inline uint64_t i64_image(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
__device__ inline uint64_t f64_image(uint64_t b) { return (b >> 63) ? ~b : (b | 0x8000000000000000ull); } // f64::total_cmp

inline uint32_t grid_for(uint64_t n) {
  const uint64_t want = (n + kOrderBlock - 1) / kOrderBlock;
  const uint64_t cap = (uint64_t)g_ctx.cu_count * 8;
  return (uint32_t)std::max<uint64_t>(1, std::min(want, cap));
}

} // namespace

} // namespace llkv
