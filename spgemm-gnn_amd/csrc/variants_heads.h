// The kernel instantiations of the multi-head aggregation (csrc/heads_aggregate.hip, namespace
// maxk_mh), as data, under the rule of variants.h: the template arguments are a POD, the compiled
// set is one constexpr table, one select_* picks the variant, and the launchers dispatch over the
// table (dispatch_variant, common.h). Plain C++17 with no HIP.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

namespace maxk_mh {

constexpr int kHeadsWave = 64;
constexpr int kHeadsThreads = 256;                     // 4 waves per work-group
constexpr int kHeadsWaves = kHeadsThreads / kHeadsWave;
constexpr int kHeadsTile = 16;                         // rows (columns) of a work-group
constexpr int kHeadsMaxHeads = 16;
constexpr int kHeadsMinLanes = 8;                      // lanes of an edge, at least
// A row (forward) or column (backward) of at most kHeadsShortMax edges is served by one lane
// group, of at most kHeadsMediumMax by one wave, a longer one by the whole work-group.
constexpr int kHeadsShortMax = 16;
constexpr int kHeadsMediumMax = 512;

namespace detail {
inline std::string name(const char* kernel, int a) {
  return std::string("maxk_mh::") + kernel + "<" + std::to_string(a) + ">";
}
inline std::string name(const char* kernel, int a, int b) {
  return std::string("maxk_mh::") + kernel + "<" + std::to_string(a) + ", " + std::to_string(b) +
         ">";
}
}  // namespace detail

// k rounded up to a power of two within [kHeadsMinLanes, kHeadsWave]: the lanes that serve one
// edge, lane `sub` holding the slots sub, sub + lanes, ... below k (more than one above k = 64)
constexpr int heads_lanes(int k) {
  int lp = kHeadsMinLanes;
  while (lp < k && lp < kHeadsWave) lp <<= 1;
  return lp;
}

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
  return detail::name("heads_fwd_kernel", x.lp);
}
inline constexpr std::array<HeadsFwdVariant, 4> kHeadsFwdVariants = {{{8}, {16}, {32}, {64}}};
constexpr HeadsFwdVariant select_heads_fwd_variant(int k) { return {heads_lanes(k)}; }

// heads_bwd_kernel<LP, HP>: LP lanes per edge, per-head reduction over HP >= num_heads head
// places (LP >= HP: the reduction ends with one head per lane)
struct HeadsBwdVariant {
  int lp, hp;
  constexpr bool operator==(const HeadsBwdVariant& o) const { return lp == o.lp && hp == o.hp; }
};
inline std::string kernel_name(const HeadsBwdVariant& x) {
  return detail::name("heads_bwd_kernel", x.lp, x.hp);
}
inline constexpr std::array<HeadsBwdVariant, 7> kHeadsBwdVariants = {
    {{8, 4}, {16, 4}, {32, 4}, {64, 4}, {16, 16}, {32, 16}, {64, 16}}};
constexpr HeadsBwdVariant select_heads_bwd_variant(int k, int num_heads) {
  const int hp = num_heads <= 4 ? 4 : 16;
  const int lp = heads_lanes(k);
  return {lp < hp ? hp : lp, hp};
}

// The selectors stay inside their tables over the whole accepted domain (1 <= k <= 256,
// 1 <= num_heads <= 16), and every table entry is selected by some input: checked where the
// tables are compiled.
namespace detail {
template <class Table, class V>
constexpr bool in_table(const Table& table, const V& v) {
  for (const V& t : table)
    if (t == v) return true;
  return false;
}
constexpr bool heads_selectors_closed() {
  bool fwd_hit[kHeadsFwdVariants.size()] = {}, bwd_hit[kHeadsBwdVariants.size()] = {};
  for (int k = 1; k <= 256; ++k) {
    if (!in_table(kHeadsFwdVariants, select_heads_fwd_variant(k))) return false;
    for (size_t i = 0; i < kHeadsFwdVariants.size(); ++i)
      if (kHeadsFwdVariants[i] == select_heads_fwd_variant(k)) fwd_hit[i] = true;
    for (int h = 1; h <= kHeadsMaxHeads; ++h) {
      const HeadsBwdVariant v = select_heads_bwd_variant(k, h);
      if (!in_table(kHeadsBwdVariants, v) || v.lp < v.hp || v.hp < h) return false;
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
