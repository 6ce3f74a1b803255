// The kernel instantiations of the neighbour sampler (csrc/sample.hip, namespace maxk_sp), as
// data, under the rule of variants.h: the template arguments are a POD, the compiled set is one
// constexpr table, one select_* picks the variant, and the launcher dispatches over the table
// (dispatch_variant, common.h). Plain C++17 with no HIP.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

namespace maxk_sp {

constexpr int kSpWave = 64;
constexpr int kSpThreads = 256;                  // 4 waves per work-group
constexpr int kSpWaves = kSpThreads / kSpWave;
constexpr int kSpTile = 16;                      // seeds of a work-group
constexpr int kSpGroup = 16;                     // lanes of a lane group: one short row each
// A row of at most kSpShortMax edges is served by one lane group, of at most kSpMediumMax by one
// wave that holds the ranks in registers (kSpSlots per lane), a longer one by the work-group.
constexpr int kSpShortMax = kSpGroup;
constexpr int kSpSlots = 8;
constexpr int kSpMediumMax = kSpWave * kSpSlots;

// sample_kernel<ALL>: ALL = every edge of every seed is kept (fanout < 0), no selection code
struct SampleVariant {
  bool all;
  constexpr bool operator==(const SampleVariant& o) const { return all == o.all; }
};
inline std::string kernel_name(const SampleVariant& x) {
  return std::string("maxk_sp::sample_kernel<") + (x.all ? "true" : "false") + ">";
}
inline constexpr std::array<SampleVariant, 2> kSampleVariants = {{{false}, {true}}};
constexpr SampleVariant select_sample_variant(int fanout) { return {fanout < 0}; }

// The selector stays inside its table over the accepted domain (any fanout but 0), and every
// entry is selected by some input: checked where the table is compiled.
namespace detail {
constexpr bool sample_selector_closed() {
  bool hit[kSampleVariants.size()] = {};
  for (int f : {-2147483647 - 1, -1, 1, 2, 10, 2147483647}) {
    const SampleVariant v = select_sample_variant(f);
    bool found = false;
    for (size_t i = 0; i < kSampleVariants.size(); ++i)
      if (kSampleVariants[i] == v) found = hit[i] = true;
    if (!found) return false;
  }
  for (bool b : hit)
    if (!b) return false;
  return true;
}
}  // namespace detail
static_assert(detail::sample_selector_closed(),
              "the sample selector leaves its table, or a table entry is never selected");

}  // namespace maxk_sp
