// The kernel instantiations of the CBSR-times-table products (csrc/cbsr_linear.hip, namespace
// maxk_lin), as data, under the rule of variants.h: the template arguments are a POD, the compiled
// set is one constexpr table per kernel family, one select_* picks the variant, and the launchers
// dispatch over the table (dispatch_variant, common.h). The geometry that the entry points,
// tools/variant_check.cpp and the tests' restatement share lives here too. Plain C++17, no HIP.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

#include "variants.h"

namespace maxk_lin {

constexpr int kLinWave = 64;
constexpr int kLinThreads = 1024;                // 16 waves per work-group, one row per wave
constexpr int kLinWaves = kLinThreads / kLinWave;
// Work-groups of one launch over all panels: a constant (the CUs of an MI355X), so that the
// number of partial sums of the weight gradient, and with it its scratch, is a function of the
// shape alone. Each work-group stages its panel once and walks row blocks from there.
constexpr int kLinGroups = 256;
// Slots whose partial dot products the sampled product reduces across the wave in one
// reduce-scatter: 15 + 2 shuffles for 16 sums
constexpr int kLinSlotTile = 16;
constexpr int kLinMaxPanels = 65535;             // panels are blockIdx.y

// The operations, as maxk_cbsr_linear_scratch_bytes numbers them
enum : int { kLinMatmul = 0, kLinSampled = 1, kLinWeightGrad = 2 };

// Panel width: the columns of the [D, M] table that a work-group holds in LDS, D * MP floats. A
// lane owns MP / 64 adjacent columns. Both widths fit the LDS at every D <= 256 (64 KB and 128 KB
// at D = 256), so D does not move the choice: a table of at most 64 columns takes the narrow
// panel, where the wide one would leave half of the lanes without a column.
constexpr int panel_width(int dim_origin, int dim_m) {
  (void)dim_origin;
  return dim_m > 64 ? 128 : 64;
}
constexpr int64_t panel_count(int dim_origin, int dim_m) {
  const int mp = panel_width(dim_origin, dim_m);
  return ((int64_t)dim_m + mp - 1) / mp;
}
// Work-groups along the rows: every wave has a row, and all panels together stay at kLinGroups
constexpr int row_groups(int64_t num_rows, int64_t panels) {
  const int64_t want = (num_rows + kLinWaves - 1) / kLinWaves;
  const int64_t cap = panels >= kLinGroups ? 1 : kLinGroups / panels;
  return (int)(want < cap ? (want < 1 ? 1 : want) : cap);
}
// Scratch of an operation in bytes; -1 outside the limits 1 <= k <= D <= 256, M >= 1, N >= 0.
//   matmul        none
//   sampled       with more than one panel, the panels' partial sums [P][N, k]
//   weight grad   the work-groups' accumulators [P][W][D, MP] and sums of values [W][D]
constexpr int64_t scratch_bytes(int op, int64_t num_rows, int dim_origin, int dim_k,
                                int dim_m) {
  if (num_rows < 0 || dim_k < 1 || dim_k > dim_origin || dim_origin > 256 || dim_m < 1) return -1;
  const int64_t p = panel_count(dim_origin, dim_m);
  if (op == kLinMatmul) return 0;
  if (op == kLinSampled) return p > 1 ? 4 * p * num_rows * dim_k : 0;
  if (op != kLinWeightGrad) return -1;
  const int64_t w = row_groups(num_rows, p);
  const int mp = panel_width(dim_origin, dim_m);
  return 4 * (p * w * dim_origin * mp + w * dim_origin);
}

// cbsr_matmul_kernel<MP>, cbsr_sampled_kernel<MP>, cbsr_weight_grad_kernel<MP>
template <int Which>
struct PanelVariant {
  int mp;
  constexpr bool operator==(const PanelVariant& o) const { return mp == o.mp; }
};
using MatmulVariant = PanelVariant<kLinMatmul>;
using SampledVariant = PanelVariant<kLinSampled>;
using WeightGradVariant = PanelVariant<kLinWeightGrad>;
inline std::string kernel_name(const MatmulVariant& x) {
  return maxk::variants_detail::name_in("maxk_lin", "cbsr_matmul_kernel", x.mp);
}
inline std::string kernel_name(const SampledVariant& x) {
  return maxk::variants_detail::name_in("maxk_lin", "cbsr_sampled_kernel", x.mp);
}
inline std::string kernel_name(const WeightGradVariant& x) {
  return maxk::variants_detail::name_in("maxk_lin", "cbsr_weight_grad_kernel", x.mp);
}
inline constexpr std::array<MatmulVariant, 2> kMatmulVariants = {{{64}, {128}}};
inline constexpr std::array<SampledVariant, 2> kSampledVariants = {{{64}, {128}}};
inline constexpr std::array<WeightGradVariant, 2> kWeightGradVariants = {{{64}, {128}}};
constexpr MatmulVariant select_matmul_variant(int dim_origin, int dim_m) {
  return {panel_width(dim_origin, dim_m)};
}
constexpr SampledVariant select_sampled_variant(int dim_origin, int dim_m) {
  return {panel_width(dim_origin, dim_m)};
}
constexpr WeightGradVariant select_weight_grad_variant(int dim_origin, int dim_m) {
  return {panel_width(dim_origin, dim_m)};
}

// The selectors stay inside their tables over D up to 256 and the widths of M around every panel
// edge, every table entry is selected, and the widest panel fits the LDS next to the sums.
namespace detail {
constexpr bool linear_selectors_closed() {
  bool hit[2] = {};
  for (int d : {1, 16, 100, 128, 129, 256})
    for (int m = 1; m <= 300; ++m) {
      const int mp = panel_width(d, m);
      if (!maxk::has_variant(kMatmulVariants, select_matmul_variant(d, m)) ||
          !maxk::has_variant(kSampledVariants, select_sampled_variant(d, m)) ||
          !maxk::has_variant(kWeightGradVariants, select_weight_grad_variant(d, m)))
        return false;
      if (mp % kLinWave != 0 || 4 * (d * mp + d) > 160 * 1024) return false;
      if (panel_count(d, m) * mp < m || (panel_count(d, m) - 1) * mp >= m) return false;
      hit[mp == 128] = true;
    }
  return hit[0] && hit[1];
}
}  // namespace detail
static_assert(detail::linear_selectors_closed(),
              "a CBSR-linear selector leaves its table, or a table entry is never selected");

}  // namespace maxk_lin
