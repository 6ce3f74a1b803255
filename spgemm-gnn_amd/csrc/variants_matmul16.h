// The kernel instantiations of the 16-bit CBSR-times-table product (csrc/cbsr_matmul16.hip,
// namespace maxk_mm16), as data, under the rule of variants.h: the template arguments are a POD,
// the compiled set is one constexpr table, one select_* picks the variant, and the launcher
// dispatches over the table (dispatch_variant, common.h). The geometry that the kernel,
// tools/variant_check.cpp, the entry points and the tests' restatement share lives here too.
// Plain C++17, no HIP.
#pragma once

#include <array>
#include <cstdint>
#include <string>

#include "variants.h"

namespace maxk_mm16 {

constexpr int kBf16 = 1;                     // MAXK_DTYPE_BF16
constexpr int kF16 = 2;                      // MAXK_DTYPE_F16

constexpr int kWave = 64;
constexpr int kThreads = 512;                // 8 waves per work-group
constexpr int kWaves = kThreads / kWave;
constexpr int kWaveRows = 16;                // rows of a tile that one wave fills, multiplies, stores
constexpr int kTileRows = kWaves * kWaveRows;  // 128
constexpr int kStep = 32;                    // depth of one v_mfma_f32_16x16x32
constexpr int kAPad = 8;                     // elements behind a densified row (bank spread, 16 B)
constexpr int kTPad = 16;                    // elements behind a staged row of the panel (32 B)
constexpr int kSlotLanes = kThreads / kTileRows;  // 4 threads share a row's slots
constexpr int kSlotsHeld = 16;               // slots a thread prefetches: k <= 64 in registers
// Work-groups of one launch over all panels: a constant (the CUs of an MI355X)
constexpr int kGroups = 256;
constexpr int kMaxPanels = 65535;            // panels are blockIdx.y
constexpr int kCuLdsBytes = 160 * 1024;

// Depth of the product: D rounded up to the next of 64, 128, 256.
constexpr int padded_dim(int dim) { return dim <= 64 ? 64 : dim <= 128 ? 128 : 256; }
// Panel width: the columns of the table, and of out, that a work-group owns.
constexpr int panel_width(int dim_m) { return dim_m > 64 ? 128 : 64; }
constexpr int64_t panel_count(int dim_m) {
  return ((int64_t)dim_m + panel_width(dim_m) - 1) / panel_width(dim_m);
}
// Work-groups along the rows a panel may have, and those it has: one per tile up to the cap
constexpr int group_cap(int64_t panels) { return panels >= kGroups ? 1 : (int)(kGroups / panels); }
constexpr int row_groups(int64_t num_rows, int64_t panels) {
  const int64_t want = (num_rows + kTileRows - 1) / kTileRows;
  const int64_t cap = group_cap(panels);
  return (int)(want < cap ? (want < 1 ? 1 : want) : cap);
}
// LDS of a work-group in bytes: the panel [DP][MP + 16] and the densified tile [128][DP + 8],
// 16-bit elements
constexpr int lds_bytes(int dp, int mp) {
  return 2 * (dp * (mp + kTPad) + kTileRows * (dp + kAPad));
}
// Waves a SIMD the kernel is compiled for. The grid is at most kGroups work-groups, one a CU, which
// is 2 waves a SIMD whatever the LDS would leave room for (4 up to 80 KB a work-group, 2 above):
// compiled for 4, the variants below 80 KB spill 8 to 80 bytes a lane for an occupancy they never
// reach.
constexpr int waves_per_simd(int dp, int mp) {
  return kCuLdsBytes / lds_bytes(dp, mp) >= 1 ? 2 : 0;
}
// Where feature f of a 32-feature step sits among the step's 32 depth positions. A lane (i, q) of
// the MFMA holds positions 8 q .. 8 q + 7; the transposing LDS read hands it four consecutive
// features a read, and the two reads take features 4 q .. and 16 + 4 q .. so that the 16 panel rows
// of one read fall on different bank groups. f = (h, q, e) in bits 4, 3-2, 1-0 goes to (q, h, e).
constexpr int depth_position(int f) { return (f & 3) | ((f >> 4) & 1) << 2 | ((f >> 2) & 3) << 3; }
// Where column c of a 32-column group of the panel is staged. The MFMA's 16 output columns of tile
// h of the group are positions 16 h + 4 q + r of lane group q, register r; they hold the columns
// 8 q + 4 h + r, so that a lane's two tiles are 8 consecutive columns of out: c = (q, h, r) in bits
// 4-3, 2, 1-0 goes to (h, q, r).
constexpr int staged_column(int c) { return (c & 3) | ((c >> 3) & 3) << 2 | ((c >> 2) & 1) << 4; }

// matmul16_kernel<DP, MP, kDtype>
struct Matmul16Variant {
  int dp, mp, dtype;
  constexpr bool operator==(const Matmul16Variant& o) const {
    return dp == o.dp && mp == o.mp && dtype == o.dtype;
  }
};
inline std::string kernel_name(const Matmul16Variant& x) {
  return maxk::variants_detail::name_in("maxk_mm16", "matmul16_kernel", x.dp, x.mp, x.dtype);
}
inline constexpr std::array<Matmul16Variant, 12> kMatmul16Variants = {{
    {64, 64, kBf16}, {64, 128, kBf16}, {128, 64, kBf16}, {128, 128, kBf16},
    {256, 64, kBf16}, {256, 128, kBf16}, {64, 64, kF16}, {64, 128, kF16},
    {128, 64, kF16}, {128, 128, kF16}, {256, 64, kF16}, {256, 128, kF16}}};
constexpr Matmul16Variant select_matmul16_variant(int dim_origin, int dim_m, int dtype) {
  return {padded_dim(dim_origin), panel_width(dim_m), dtype};
}

// The selector stays inside the table over every D up to 256, the widths of M around every panel
// edge and both types, every entry is selected, one work-group of the widest variant fits a CU's
// 160 KB of LDS, and the two placements are permutations.
namespace detail {
constexpr bool matmul16_selector_closed() {
  bool hit[3][2][2] = {};
  for (int d = 1; d <= 256; ++d)
    for (int m : {1, 63, 64, 65, 128, 129, 256, 257, 300})
      for (int dt = kBf16; dt <= kF16; ++dt) {
        const Matmul16Variant v = select_matmul16_variant(d, m, dt);
        if (!maxk::has_variant(kMatmul16Variants, v)) return false;
        if (v.dp < d || (v.dp > 64 && v.dp / 2 >= d)) return false;
        if (panel_count(m) * v.mp < m || (panel_count(m) - 1) * v.mp >= m) return false;
        if (lds_bytes(v.dp, v.mp) > kCuLdsBytes) return false;
        hit[v.dp == 64 ? 0 : v.dp == 128 ? 1 : 2][v.mp == 128][dt - kBf16] = true;
      }
  uint32_t depth = 0, column = 0;
  for (int r = 0; r < kStep; ++r) {
    depth |= 1u << depth_position(r);
    column |= 1u << staged_column(r);
  }
  if (depth != 0xffffffffu || column != 0xffffffffu) return false;
  for (auto& h : hit)
    for (auto& g : h)
      if (!g[0] || !g[1]) return false;
  return true;
}
}  // namespace detail
static_assert(detail::matmul16_selector_closed(),
              "the matmul16 selector leaves its table, or a table entry is never selected");

}  // namespace maxk_mm16
