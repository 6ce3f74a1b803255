// The kernel instantiations of the multi-head aggregation (csrc/heads_aggregate.hip, namespace
// maxk_mh), as data, under the rule of variants.h: the template arguments are a POD, the compiled
// set is one constexpr table, one select_* picks the variant, and the launchers dispatch over the
// table (dispatch_variant, common.h). Plain C++17 with no HIP.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

#include "lane_groups.h"

namespace maxk_mh {

namespace lg = maxk::lg;  // the geometry: lanes of an edge, tile, row limits

constexpr int kHeadsMaxHeads = 16;

// The head of feature s is s / F. The kernels compute it as (s * heads_magic(F)) >> 16, exact for
// every s < 256 and 4 <= F <= 256: the error s / 65536 < 1 / 256 <= 1 / F never reaches the next
// integer from a fractional part of at most 1 - 1 / F.
constexpr uint32_t heads_magic(int f) { return 65536u / (uint32_t)f + 1u; }
constexpr int heads_head_of(int s, uint32_t magic) { return (int)(((uint32_t)s * magic) >> 16); }

// heads_fwd_kernel<LP>: LP lanes per edge
struct HeadsFwdVariant {
  int lp;
  constexpr bool operator==(const HeadsFwdVariant& o) const { return lp == o.lp; }
};
inline std::string kernel_name(const HeadsFwdVariant& x) {
  return maxk::variants_detail::name_in("maxk_mh", "heads_fwd_kernel", x.lp);
}
inline constexpr std::array<HeadsFwdVariant, 4> kHeadsFwdVariants = {{{8}, {16}, {32}, {64}}};
constexpr HeadsFwdVariant select_heads_fwd_variant(int k) { return {lg::lanes(k)}; }

// heads_bwd_kernel<LP, HP>: LP lanes per edge, per-head reduction over HP >= num_heads head
// places (LP >= HP: the reduction ends with one head per lane)
struct HeadsBwdVariant {
  int lp, hp;
  constexpr bool operator==(const HeadsBwdVariant& o) const { return lp == o.lp && hp == o.hp; }
};
inline std::string kernel_name(const HeadsBwdVariant& x) {
  return maxk::variants_detail::name_in("maxk_mh", "heads_bwd_kernel", x.lp, x.hp);
}
inline constexpr std::array<HeadsBwdVariant, 7> kHeadsBwdVariants = {
    {{8, 4}, {16, 4}, {32, 4}, {64, 4}, {16, 16}, {32, 16}, {64, 16}}};
constexpr HeadsBwdVariant select_heads_bwd_variant(int k, int num_heads) {
  const int hp = num_heads <= 4 ? 4 : 16;
  const int lp = lg::lanes(k);
  return {lp < hp ? hp : lp, hp};
}

// The selectors stay inside their tables over the whole accepted domain (1 <= k <= 256,
// 1 <= num_heads <= 16), and every table entry is selected by some input: checked where the
// tables are compiled.
namespace detail {
constexpr bool heads_selectors_closed() {
  bool fwd_hit[kHeadsFwdVariants.size()] = {}, bwd_hit[kHeadsBwdVariants.size()] = {};
  for (int k = 1; k <= 256; ++k) {
    if (!maxk::has_variant(kHeadsFwdVariants, select_heads_fwd_variant(k))) return false;
    for (size_t i = 0; i < kHeadsFwdVariants.size(); ++i)
      if (kHeadsFwdVariants[i] == select_heads_fwd_variant(k)) fwd_hit[i] = true;
    for (int h = 1; h <= kHeadsMaxHeads; ++h) {
      const HeadsBwdVariant v = select_heads_bwd_variant(k, h);
      if (!maxk::has_variant(kHeadsBwdVariants, v) || v.lp < v.hp || v.hp < h) return false;
      for (size_t i = 0; i < kHeadsBwdVariants.size(); ++i)
        if (kHeadsBwdVariants[i] == v) bwd_hit[i] = true;
    }
  }
  for (bool b : fwd_hit)
    if (!b) return false;
  for (bool b : bwd_hit)
    if (!b) return false;
  return true;
}
}  // namespace detail
static_assert(detail::heads_selectors_closed(),
              "a heads selector leaves its table, or a table entry is never selected");

}  // namespace maxk_mh
