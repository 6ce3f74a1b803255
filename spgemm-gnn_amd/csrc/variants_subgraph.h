// The kernel instantiations of the induced-subgraph extraction (csrc/subgraph.hip, namespace
// maxk_sg), as data, under the rule of variants.h: the template arguments are a POD, the compiled
// set is one constexpr table, one select_* picks the variant, and the launcher dispatches over the
// table (dispatch_variant, common.h). Plain C++17 with no HIP.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

namespace maxk_sg {

constexpr int kSgWave = 64;
constexpr int kSgThreads = 256;                  // 4 waves per work-group
constexpr int kSgWaves = kSgThreads / kSgWave;
constexpr int kSgTile = 16;                      // positions of `nodes` per work-group
constexpr int kSgGroup = 16;                     // lanes of a lane group: one short row each
// A lane reads its edges as quads (one 16-byte load of idx, four mark gathers); a wave covers
// kSgQuad * kSgWave consecutive edges per chunk, counted from the 16-byte boundary at or below
// the row's first edge.
constexpr int kSgQuad = 4;
constexpr int kSgChunk = kSgQuad * kSgWave;
// A row of at most kSgShortMax edges is served by one lane group, of at most kSgMediumMax by one
// wave in kSgMediumChunks chunks (the row and the up to kSgQuad - 1 edges of alignment in front of
// it), a longer one by the work-group, kSgHubChunks chunks per wave and pass.
constexpr int kSgShortMax = kSgGroup;
constexpr int kSgMediumMax = 512;
constexpr int kSgMediumChunks = (kSgMediumMax + kSgQuad - 1 + kSgChunk - 1) / kSgChunk;
constexpr int kSgHubChunks = 2;
constexpr int kSgHubPass = kSgWaves * kSgHubChunks * kSgChunk;   // edges of a work-group pass

// subgraph_rows_kernel<FILL>: false counts the kept edges of every position (out_ptr before its
// scan), true places them (out_col, out_eid) behind the scanned out_ptr
struct SubgraphVariant {
  bool fill;
  constexpr bool operator==(const SubgraphVariant& o) const { return fill == o.fill; }
};
inline std::string kernel_name(const SubgraphVariant& x) {
  return std::string("maxk_sg::subgraph_rows_kernel<") + (x.fill ? "true" : "false") + ">";
}
inline constexpr std::array<SubgraphVariant, 2> kSubgraphVariants = {{{false}, {true}}};
constexpr SubgraphVariant select_subgraph_variant(bool fill) { return {fill}; }

// The selector stays inside its table over its whole domain, and every entry is selected by some
// input: checked where the table is compiled.
namespace detail {
constexpr bool subgraph_selector_closed() {
  bool hit[kSubgraphVariants.size()] = {};
  for (bool f : {false, true}) {
    const SubgraphVariant v = select_subgraph_variant(f);
    bool found = false;
    for (size_t i = 0; i < kSubgraphVariants.size(); ++i)
      if (kSubgraphVariants[i] == v) found = hit[i] = true;
    if (!found) return false;
  }
  for (bool b : hit)
    if (!b) return false;
  return true;
}
}  // namespace detail
static_assert(detail::subgraph_selector_closed(),
              "the subgraph selector leaves its table, or a table entry is never selected");

}  // namespace maxk_sg
