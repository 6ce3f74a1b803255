// The kernel instantiations of the max aggregation (csrc/max_aggregate.hip, namespace maxk_mx),
// as data, under the rule of variants.h: the template arguments are a POD, the compiled set is
// one constexpr table, one select_* picks the variant, and the launchers dispatch over the table
// (dispatch_variant, common.h). Plain C++17 with no HIP.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

namespace maxk_mx {

constexpr int kMaxWave = 64;
constexpr int kMaxThreads = 256;                    // 4 waves per work-group
constexpr int kMaxWaves = kMaxThreads / kMaxWave;
constexpr int kMaxTile = 16;                        // rows (columns) of a work-group
constexpr int kMaxMinLanes = 8;                     // lanes of an edge, at least
// A row (forward) or column (backward) of at most kMaxShortMax edges is served by one lane
// group, of at most kMaxMediumMax by one wave, a longer one by the whole work-group.
constexpr int kMaxShortMax = 16;
constexpr int kMaxMediumMax = 512;
// The forward packs an edge's place in its row into 24 bits of the LDS cell.
constexpr int64_t kMaxRowEdges = (int64_t)1 << 24;

namespace detail {
inline std::string name(const char* kernel, int a) {
  return std::string("maxk_mx::") + kernel + "<" + std::to_string(a) + ">";
}
inline std::string name(const char* kernel, int a, bool b) {
  return std::string("maxk_mx::") + kernel + "<" + std::to_string(a) + ", " +
         (b ? "true" : "false") + ">";
}
}  // namespace detail

// k rounded up to a power of two within [kMaxMinLanes, kMaxWave]: the lanes that serve one edge,
// lane `sub` holding the slots sub, sub + lanes, ... below k (more than one above k = 64)
constexpr int max_lanes(int k) {
  int lp = kMaxMinLanes;
  while (lp < k && lp < kMaxWave) lp <<= 1;
  return lp;
}

// Row states of the forward's LDS: one per lane group that serves a short row at a time
constexpr int max_fwd_states(int lp) {
  const int ng = kMaxThreads / lp;
  return ng < kMaxTile ? ng : kMaxTile;
}

// max_fwd_kernel<LP, ARG>: LP lanes per edge; ARG: arg_edge / arg_slot are written
struct MaxFwdVariant {
  int lp;
  bool arg;
  constexpr bool operator==(const MaxFwdVariant& o) const { return lp == o.lp && arg == o.arg; }
};
inline std::string kernel_name(const MaxFwdVariant& x) {
  return detail::name("max_fwd_kernel", x.lp, x.arg);
}
inline constexpr std::array<MaxFwdVariant, 8> kMaxFwdVariants = {
    {{8, false}, {16, false}, {32, false}, {64, false}, {8, true}, {16, true}, {32, true},
     {64, true}}};
constexpr MaxFwdVariant select_max_fwd_variant(int k, bool arg) { return {max_lanes(k), arg}; }

// max_bwd_kernel<LP>: LP lanes per transposed entry
struct MaxBwdVariant {
  int lp;
  constexpr bool operator==(const MaxBwdVariant& o) const { return lp == o.lp; }
};
inline std::string kernel_name(const MaxBwdVariant& x) {
  return detail::name("max_bwd_kernel", x.lp);
}
inline constexpr std::array<MaxBwdVariant, 4> kMaxBwdVariants = {{{8}, {16}, {32}, {64}}};
constexpr MaxBwdVariant select_max_bwd_variant(int k) { return {max_lanes(k)}; }

// The selectors stay inside their tables over the whole accepted domain (1 <= k <= 256, with
// and without arg_*), and every table entry is selected by some input: checked where the tables
// are compiled.
namespace detail {
template <class Table, class V>
constexpr bool in_table(const Table& table, const V& v) {
  for (const V& t : table)
    if (t == v) return true;
  return false;
}
constexpr bool max_selectors_closed() {
  bool fwd_hit[kMaxFwdVariants.size()] = {}, bwd_hit[kMaxBwdVariants.size()] = {};
  for (int k = 1; k <= 256; ++k) {
    for (int arg = 0; arg < 2; ++arg) {
      const MaxFwdVariant v = select_max_fwd_variant(k, arg != 0);
      if (!in_table(kMaxFwdVariants, v)) return false;
      for (size_t i = 0; i < kMaxFwdVariants.size(); ++i)
        if (kMaxFwdVariants[i] == v) fwd_hit[i] = true;
    }
    if (!in_table(kMaxBwdVariants, select_max_bwd_variant(k))) return false;
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
