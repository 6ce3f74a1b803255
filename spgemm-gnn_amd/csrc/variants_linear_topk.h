// The kernel instantiations of the fused linear + top-k (csrc/linear_topk.hip, namespace maxk_lt),
// as data, under the rule of variants.h: the template arguments are a POD, the compiled set is one
// constexpr table, one select_* picks the variant, and the launcher dispatches over the table
// (dispatch_variant, common.h). The geometry that the kernel, tools/variant_check.cpp and the
// documents share lives here too. Plain C++17, no HIP.
#pragma once

#include <array>
#include <cstdint>
#include <string>

#include "variants.h"

namespace maxk_lt {

constexpr int kLtWave = 64;
constexpr int kLtThreads = 256;                // 4 waves per work-group
constexpr int kLtWaves = kLtThreads / kLtWave;
constexpr int kLtWaveRows = 16;                // rows of an MFMA tile: a wave's rows
constexpr int kLtTileRows = kLtWaves * kLtWaveRows;  // 64 rows per work-group
constexpr int kLtChunk = 32;                   // KC: columns of D_in staged per step
constexpr int kLtChunkPad = 4;                 // floats behind a staged row (bank spread, 16 B)
constexpr int kLtRowFloats = kLtChunk + kLtChunkPad;
constexpr int kLtEpiRows = 4;                  // rows a wave turns round in LDS at a time
constexpr int kLtEpiPad = 16;                  // floats behind a turned row

// Column count of the accumulators: D rounded up to the next of 64, 128, 256.
constexpr int padded_dim(int dim) { return dim <= 64 ? 64 : dim <= 128 ? 128 : 256; }

// LDS of a work-group in bytes: the staged chunks h [64][36] and W [DP][36] while the product runs,
// then, in the same bytes, each wave's turned rows, histogram and emission rows.
constexpr int stage_bytes(int dp) { return 4 * (kLtTileRows + dp) * kLtRowFloats; }
constexpr int wave_epilogue_bytes(int dp) {
  return 4 * kLtEpiRows * (dp + kLtEpiPad) + 4 * 256 + 4 * 256 + 256;
}
constexpr int lds_bytes(int dp) {
  const int a = stage_bytes(dp), b = kLtWaves * wave_epilogue_bytes(dp);
  return a > b ? a : b;
}

// linear_topk_kernel<DP, kDense>
struct LinearTopkVariant {
  int dp;
  bool dense;
  constexpr bool operator==(const LinearTopkVariant& o) const {
    return dp == o.dp && dense == o.dense;
  }
};
inline std::string kernel_name(const LinearTopkVariant& x) {
  return maxk::variants_detail::name_in("maxk_lt", "linear_topk_kernel", x.dp, x.dense);
}
inline constexpr std::array<LinearTopkVariant, 6> kLinearTopkVariants = {{
    {64, false}, {64, true}, {128, false}, {128, true}, {256, false}, {256, true}}};
constexpr LinearTopkVariant select_linear_topk_variant(int dim, bool dense) {
  return {padded_dim(dim), dense};
}

// The selector stays inside the table over every D up to 256, every entry is selected, the
// accumulators cover D, and two work-groups of the widest variant fit a CU's 160 KB of LDS.
namespace detail {
constexpr bool linear_topk_selector_closed() {
  bool hit[3][2] = {};
  for (int d = 1; d <= 256; ++d)
    for (int dense = 0; dense < 2; ++dense) {
      const LinearTopkVariant v = select_linear_topk_variant(d, dense != 0);
      if (!maxk::has_variant(kLinearTopkVariants, v)) return false;
      if (v.dp < d || v.dp % 64 != 0 || v.dp > 256 || (v.dp > 64 && v.dp / 2 >= d)) return false;
      if (2 * lds_bytes(v.dp) > 160 * 1024 || lds_bytes(v.dp) > 64 * 1024) return false;
      hit[v.dp == 64 ? 0 : v.dp == 128 ? 1 : 2][dense] = true;
    }
  for (auto& h : hit)
    if (!h[0] || !h[1]) return false;
  return true;
}
}  // namespace detail
static_assert(detail::linear_topk_selector_closed(),
              "the linear-topk selector leaves its table, or a table entry is never selected");

}  // namespace maxk_lt
