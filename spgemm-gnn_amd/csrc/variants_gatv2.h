// The kernel instantiations of the MaxK GATv2 attention (csrc/gatv2_attention.hip, namespace
// maxk_v2), as data, under the rule of variants.h: the template arguments are a POD, the compiled
// set is one constexpr table, one select_* picks the variant, and the launchers dispatch over the
// table (dispatch_variant, common.h). Plain C++17 with no HIP.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

#include "variants_heads.h"

namespace maxk_v2 {

namespace lg = maxk::lg;  // the geometry: lanes of an edge, tile, row limits

constexpr int kGatv2MaxHeads = maxk_mh::kHeadsMaxHeads;
// work-groups of the row backward, each of which leaves one partial sum of grad_attn: a constant,
// so that the partials' count, and with it the bits of grad_attn, is a function of num_rows alone
constexpr int kGatv2MaxPartials = 1024;

// The head of feature s is s / F, computed as (s * heads_magic(F)) >> 16 (variants_heads.h). Here
// F may be any of 1 .. 256: the product exceeds s * 65536 / F by at most s / 65536 < 1 / 256 <=
// 1 / F, which never reaches the next integer from a fractional part of at most 1 - 1 / F.
using maxk_mh::heads_head_of;
using maxk_mh::heads_magic;

// gatv2_score_fwd_kernel<LP, HP>: LP lanes per edge, per-head reduction over HP >= num_heads head
// places (LP >= HP: the reduce-scatter ends with one head per lane), as heads_bwd_kernel<LP, HP>
struct ScoreFwdVariant {
  int lp, hp;
  constexpr bool operator==(const ScoreFwdVariant& o) const { return lp == o.lp && hp == o.hp; }
};
inline std::string kernel_name(const ScoreFwdVariant& x) {
  return maxk::variants_detail::name_in("maxk_v2", "gatv2_score_fwd_kernel", x.lp, x.hp);
}
inline constexpr std::array<ScoreFwdVariant, 7> kScoreFwdVariants = {
    {{8, 4}, {16, 4}, {32, 4}, {64, 4}, {16, 16}, {32, 16}, {64, 16}}};
constexpr ScoreFwdVariant select_score_fwd_variant(int k, int num_heads) {
  const int hp = num_heads <= 4 ? 4 : 16;
  const int lp = lg::lanes(k);
  return {lp < hp ? hp : lp, hp};
}

// gatv2_score_bwd_rows_kernel<LP> and gatv2_score_bwd_cols_kernel<LP>: LP lanes per edge; both
// gather grad_logits by the slot's own head and reduce nothing per head
template <int Which>
struct LanesVariant {
  int lp;
  constexpr bool operator==(const LanesVariant& o) const { return lp == o.lp; }
};
using ScoreRowsVariant = LanesVariant<0>;
using ScoreColsVariant = LanesVariant<1>;
inline std::string kernel_name(const ScoreRowsVariant& x) {
  return maxk::variants_detail::name_in("maxk_v2", "gatv2_score_bwd_rows_kernel", x.lp);
}
inline std::string kernel_name(const ScoreColsVariant& x) {
  return maxk::variants_detail::name_in("maxk_v2", "gatv2_score_bwd_cols_kernel", x.lp);
}
inline constexpr std::array<ScoreRowsVariant, 4> kScoreRowsVariants = {{{8}, {16}, {32}, {64}}};
inline constexpr std::array<ScoreColsVariant, 4> kScoreColsVariants = {{{8}, {16}, {32}, {64}}};
constexpr ScoreRowsVariant select_score_rows_variant(int k) { return {lg::lanes(k)}; }
constexpr ScoreColsVariant select_score_cols_variant(int k) { return {lg::lanes(k)}; }

// The selectors stay inside their tables over the whole accepted domain (1 <= k <= 256,
// 1 <= num_heads <= 16), and every table entry is selected by some input.
namespace detail {
constexpr bool gatv2_selectors_closed() {
  bool fwd_hit[kScoreFwdVariants.size()] = {}, lanes_hit[kScoreRowsVariants.size()] = {};
  for (int k = 1; k <= 256; ++k) {
    const int lp = lg::lanes(k);
    if (!maxk::has_variant(kScoreRowsVariants, select_score_rows_variant(k)) ||
        !maxk::has_variant(kScoreColsVariants, select_score_cols_variant(k)))
      return false;
    for (size_t i = 0; i < kScoreRowsVariants.size(); ++i)
      if (kScoreRowsVariants[i].lp == lp && kScoreColsVariants[i].lp == lp) lanes_hit[i] = true;
    for (int h = 1; h <= kGatv2MaxHeads; ++h) {
      const ScoreFwdVariant v = select_score_fwd_variant(k, h);
      if (!maxk::has_variant(kScoreFwdVariants, v) || v.lp < v.hp || v.hp < h) return false;
      for (size_t i = 0; i < kScoreFwdVariants.size(); ++i)
        if (kScoreFwdVariants[i] == v) fwd_hit[i] = true;
    }
  }
  for (bool b : fwd_hit)
    if (!b) return false;
  for (bool b : lanes_hit)
    if (!b) return false;
  return true;
}
}  // namespace detail
static_assert(detail::gatv2_selectors_closed(),
              "a GATv2 selector leaves its table, or a table entry is never selected");

}  // namespace maxk_v2
