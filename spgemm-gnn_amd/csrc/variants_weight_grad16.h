// The kernel instantiations of the 16-bit weight gradient of the fused linear + MaxK
// (csrc/cbsr_weight_grad16.hip, namespace maxk_wg16), as data, under the rule of variants.h: the
// template arguments are a POD, the compiled set is one constexpr table, one select_* picks the
// variant, and the launcher dispatches over the table (dispatch_variant, common.h). The geometry
// that the kernel, tools/variant_check.cpp, the entry points and the tests' restatement share
// lives here too. Plain C++17, no HIP.
#pragma once

#include <array>
#include <cstdint>
#include <string>

#include "variants.h"

namespace maxk_wg16 {

constexpr int kBf16 = 1;                     // MAXK_DTYPE_BF16
constexpr int kF16 = 2;                      // MAXK_DTYPE_F16

constexpr int kWave = 64;
constexpr int kThreads = 512;                // 8 waves per work-group
constexpr int kWaves = kThreads / kWave;
constexpr int kChunkRows = 64;               // rows of a chunk: two MFMA depths
constexpr int kStep = 32;                    // depth of one v_mfma_f32_16x16x32
constexpr int kAPad = 8;                     // elements behind a row of A^T (bank spread, 16 B)
constexpr int kARow = kChunkRows + kAPad;    // 72 elements, 36 words
constexpr int kGPad = 16;                    // elements behind a staged row of g (32 B)
constexpr int kSlotLanes = 8;                // threads that share a row's slots
constexpr int kSlotsHeld = 8;                // slots a thread prefetches: k <= 64 in registers
// Work-groups of one launch over all panels: a constant (the CUs of an MI355X), so that the number
// of partial tables, and with it the scratch, is a function of the shape alone.
constexpr int kGroups = 256;
constexpr int kMaxPanels = 65535;            // panels are blockIdx.y

// Feature count of the A^T tile: D rounded up to the next of 64, 128, 256.
constexpr int padded_dim(int dim) { return dim <= 64 ? 64 : dim <= 128 ? 128 : 256; }
// Panel width: the columns of g, and of the [D, M] gradient, that a work-group owns.
constexpr int panel_width(int dim_m) { return dim_m > 64 ? 128 : 64; }
constexpr int64_t panel_count(int dim_m) {
  return ((int64_t)dim_m + panel_width(dim_m) - 1) / panel_width(dim_m);
}
// Work-groups along the rows a panel may have, and those it has: one per chunk up to the cap
constexpr int group_cap(int64_t panels) { return panels >= kGroups ? 1 : (int)(kGroups / panels); }
constexpr int row_groups(int64_t num_rows, int64_t panels) {
  const int64_t want = (num_rows + kChunkRows - 1) / kChunkRows;
  const int64_t cap = group_cap(panels);
  return (int)(want < cap ? (want < 1 ? 1 : want) : cap);
}
// The 8 waves as WF groups along the features times WC along the panel's columns: a wave owns whole
// 16 x 16 tiles, so 64 features (4 tiles) leave two waves to share a feature tile's columns.
constexpr int waves_along_features(int dp) { return dp / 16 < kWaves ? dp / 16 : kWaves; }
// LDS of a work-group in bytes: A^T [DP][72] and the chunk of g [64][MP + 16], 16-bit elements
constexpr int lds_bytes(int dp, int mp) { return 2 * (dp * kARow + kChunkRows * (mp + kGPad)); }
// Scratch in bytes: the work-groups' partial tables [P][W][D, MP] and sums [W][D], f32; -1 outside
// the limits 1 <= k <= D <= 256, M >= 1, N >= 0.
constexpr int64_t scratch_bytes(int64_t num_rows, int dim_origin, int dim_k, int dim_m) {
  if (num_rows < 0 || dim_k < 1 || dim_k > dim_origin || dim_origin > 256 || dim_m < 1) return -1;
  const int64_t p = panel_count(dim_m), w = row_groups(num_rows, p);
  return 4 * (p * w * dim_origin * panel_width(dim_m) + w * dim_origin);
}
// Where row r of a 32-row step sits among the step's 32 depth positions. A lane (i, q) of the MFMA
// holds positions 8 q .. 8 q + 7; the transposing LDS read hands it four consecutive rows a read,
// and the two reads take rows 4 q .. and 16 + 4 q .. so that the 16 rows of one read fall on
// different bank groups. r = (h, q, e) in bits 4, 3-2, 1-0 goes to position (q, h, e).
constexpr int depth_position(int r) { return (r & 3) | ((r >> 4) & 1) << 2 | ((r >> 2) & 3) << 3; }

// weight_grad16_kernel<DP, MP, kDtype>
struct WeightGrad16Variant {
  int dp, mp, dtype;
  constexpr bool operator==(const WeightGrad16Variant& o) const {
    return dp == o.dp && mp == o.mp && dtype == o.dtype;
  }
};
inline std::string kernel_name(const WeightGrad16Variant& x) {
  return maxk::variants_detail::name_in("maxk_wg16", "weight_grad16_kernel", x.dp, x.mp, x.dtype);
}
inline constexpr std::array<WeightGrad16Variant, 12> kWeightGrad16Variants = {{
    {64, 64, kBf16}, {64, 128, kBf16}, {128, 64, kBf16}, {128, 128, kBf16},
    {256, 64, kBf16}, {256, 128, kBf16}, {64, 64, kF16}, {64, 128, kF16},
    {128, 64, kF16}, {128, 128, kF16}, {256, 64, kF16}, {256, 128, kF16}}};
constexpr WeightGrad16Variant select_weight_grad16_variant(int dim_origin, int dim_m, int dtype) {
  return {padded_dim(dim_origin), panel_width(dim_m), dtype};
}

// The selector stays inside the table over every D up to 256, the widths of M around every panel
// edge and both types, every entry is selected, the waves tile the accumulator exactly, the depth
// positions are a permutation, and two work-groups of the widest variant fit a CU's 160 KB of LDS.
namespace detail {
constexpr bool weight_grad16_selector_closed() {
  bool hit[3][2][2] = {};
  for (int d = 1; d <= 256; ++d)
    for (int m : {1, 63, 64, 65, 128, 129, 256, 257, 300})
      for (int dt = kBf16; dt <= kF16; ++dt) {
        const WeightGrad16Variant v = select_weight_grad16_variant(d, m, dt);
        if (!maxk::has_variant(kWeightGrad16Variants, v)) return false;
        if (v.dp < d || (v.dp > 64 && v.dp / 2 >= d)) return false;
        if (panel_count(m) * v.mp < m || (panel_count(m) - 1) * v.mp >= m) return false;
        const int wf = waves_along_features(v.dp), wc = kWaves / wf;
        if ((v.dp / 16) % wf != 0 || (v.mp / 16) % wc != 0) return false;
        if (2 * lds_bytes(v.dp, v.mp) > 160 * 1024 || lds_bytes(v.dp, v.mp) > 64 * 1024) return false;
        hit[v.dp == 64 ? 0 : v.dp == 128 ? 1 : 2][v.mp == 128][dt - kBf16] = true;
      }
  uint32_t seen = 0;
  for (int r = 0; r < kStep; ++r) seen |= 1u << depth_position(r);
  if (seen != 0xffffffffu) return false;
  for (auto& h : hit)
    for (auto& g : h)
      if (!g[0] || !g[1]) return false;
  return true;
}
}  // namespace detail
static_assert(detail::weight_grad16_selector_closed(),
              "the weight-grad16 selector leaves its table, or a table entry is never selected");

}  // namespace maxk_wg16
