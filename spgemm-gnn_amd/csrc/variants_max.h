// The kernel instantiations of the max aggregation (csrc/max_aggregate.hip, namespace maxk_mx),
// as data, under the rule of variants.h: the template arguments are a POD, the compiled set is
// one constexpr table, one select_* picks the variant, and the launchers dispatch over the table
// (dispatch_variant, common.h). Plain C++17 with no HIP.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

#include "lane_groups.h"

namespace maxk_mx {

namespace lg = maxk::lg;  // the geometry: lanes of an edge, tile, row limits

// The forward packs an edge's place in its row into 24 bits of the LDS cell.
constexpr int64_t kMaxRowEdges = (int64_t)1 << 24;

// Row states of the forward's LDS: one per lane group that serves a short row at a time
constexpr int max_fwd_states(int lp) {
  const int ng = lg::kThreads / lp;
  return ng < lg::kTile ? ng : lg::kTile;
}

// max_fwd_kernel<LP, ARG>: LP lanes per edge; ARG: arg_edge / arg_slot are written
struct MaxFwdVariant {
  int lp;
  bool arg;
  constexpr bool operator==(const MaxFwdVariant& o) const { return lp == o.lp && arg == o.arg; }
};
inline std::string kernel_name(const MaxFwdVariant& x) {
  return maxk::variants_detail::name_in("maxk_mx", "max_fwd_kernel", x.lp, x.arg);
}
inline constexpr std::array<MaxFwdVariant, 8> kMaxFwdVariants = {
    {{8, false}, {16, false}, {32, false}, {64, false}, {8, true}, {16, true}, {32, true},
     {64, true}}};
constexpr MaxFwdVariant select_max_fwd_variant(int k, bool arg) { return {lg::lanes(k), arg}; }

// max_bwd_kernel<LP>: LP lanes per transposed entry
struct MaxBwdVariant {
  int lp;
  constexpr bool operator==(const MaxBwdVariant& o) const { return lp == o.lp; }
};
inline std::string kernel_name(const MaxBwdVariant& x) {
  return maxk::variants_detail::name_in("maxk_mx", "max_bwd_kernel", x.lp);
}
inline constexpr std::array<MaxBwdVariant, 4> kMaxBwdVariants = {{{8}, {16}, {32}, {64}}};
constexpr MaxBwdVariant select_max_bwd_variant(int k) { return {lg::lanes(k)}; }

// The selectors stay inside their tables over the whole accepted domain (1 <= k <= 256, with
// and without arg_*), and every table entry is selected by some input: checked where the tables
// are compiled.
namespace detail {
constexpr bool max_selectors_closed() {
  bool fwd_hit[kMaxFwdVariants.size()] = {}, bwd_hit[kMaxBwdVariants.size()] = {};
  for (int k = 1; k <= 256; ++k) {
    for (int arg = 0; arg < 2; ++arg) {
      const MaxFwdVariant v = select_max_fwd_variant(k, arg != 0);
      if (!maxk::has_variant(kMaxFwdVariants, v)) return false;
      for (size_t i = 0; i < kMaxFwdVariants.size(); ++i)
        if (kMaxFwdVariants[i] == v) fwd_hit[i] = true;
    }
    if (!maxk::has_variant(kMaxBwdVariants, select_max_bwd_variant(k))) return false;
    for (size_t i = 0; i < kMaxBwdVariants.size(); ++i)
      if (kMaxBwdVariants[i] == select_max_bwd_variant(k)) bwd_hit[i] = true;
  }
  for (bool b : fwd_hit)
    if (!b) return false;
  for (bool b : bwd_hit)
    if (!b) return false;
  return true;
}
}  // namespace detail
static_assert(detail::max_selectors_closed(),
              "a max selector leaves its table, or a table entry is never selected");

}  // namespace maxk_mx
