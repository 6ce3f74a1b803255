// The kernel instantiations of the fused linear + top-k on 16-bit operands (csrc/linear_topk16.hip,
// namespace maxk_lt16), as data, under the rule of variants.h: the template arguments are a POD,
// the compiled set is one constexpr table, one select_* picks the variant, and the launcher
// dispatches over the table (dispatch_variant, common.h). The geometry that the kernel,
// tools/variant_check.cpp and the documents share lives here too. Plain C++17, no HIP.
#pragma once

#include <array>
#include <cstdint>
#include <string>

#include "variants.h"

namespace maxk_lt16 {

constexpr int kBf16 = 1;                       // MAXK_DTYPE_BF16
constexpr int kF16 = 2;                        // MAXK_DTYPE_F16

constexpr int kWave = 64;
constexpr int kThreads = 512;                  // 8 waves per work-group
constexpr int kWaves = kThreads / kWave;
constexpr int kWaveRows = 16;                  // rows of an MFMA tile: a wave's rows
constexpr int kTileRows = kWaves * kWaveRows;  // 128 rows per work-group
constexpr int kChunk = 64;                     // KC: elements of D_in staged per step (128 bytes)
constexpr int kChunkPad = 8;                   // elements behind a staged row (bank spread, 16 B)
constexpr int kRowElems = kChunk + kChunkPad;  // 72 elements, 36 words
constexpr int kStep = 32;                      // depth of one v_mfma_f32_16x16x32
constexpr int kLoadRows = kThreads / 8;        // rows that one round of 16-byte loads covers
constexpr int kEpiRows = 4;                    // rows a wave turns round in LDS at a time
constexpr int kEpiPad = 16;                    // floats behind a turned row

// Column count of the accumulators: D rounded up to the next of 64, 128, 256.
constexpr int padded_dim(int dim) { return dim <= 64 ? 64 : dim <= 128 ? 128 : 256; }

// LDS of a work-group in bytes: the staged chunks h [128][72] and W [DP][72] of 16-bit elements
// while the product runs, then, in the same bytes, each wave's turned rows (f32), histogram and
// emission rows.
constexpr int stage_bytes(int dp) { return 2 * (kTileRows + dp) * kRowElems; }
constexpr int wave_epilogue_bytes(int dp) {
  return 4 * kEpiRows * (dp + kEpiPad) + 4 * 256 + 4 * 256 + 256;
}
constexpr int lds_bytes(int dp) {
  const int a = stage_bytes(dp), b = kWaves * wave_epilogue_bytes(dp);
  return a > b ? a : b;
}

// linear_topk16_kernel<DP, kDense, kDtype>
struct LinearTopk16Variant {
  int dp;
  bool dense;
  int dtype;
  constexpr bool operator==(const LinearTopk16Variant& o) const {
    return dp == o.dp && dense == o.dense && dtype == o.dtype;
  }
};
inline std::string kernel_name(const LinearTopk16Variant& x) {
  return maxk::variants_detail::name_in("maxk_lt16", "linear_topk16_kernel", x.dp, x.dense,
                                        x.dtype);
}
inline constexpr std::array<LinearTopk16Variant, 12> kLinearTopk16Variants = {{
    {64, false, kBf16}, {64, true, kBf16}, {128, false, kBf16}, {128, true, kBf16},
    {256, false, kBf16}, {256, true, kBf16}, {64, false, kF16}, {64, true, kF16},
    {128, false, kF16}, {128, true, kF16}, {256, false, kF16}, {256, true, kF16}}};
constexpr LinearTopk16Variant select_linear_topk16_variant(int dim, bool dense, int dtype) {
  return {padded_dim(dim), dense, dtype};
}

// The selector stays inside the table over every D up to 256 and both types, every entry is
// selected, the accumulators cover D, a round of loads covers whole rows of the stage, and two
// work-groups of the widest variant fit a CU's 160 KB of LDS.
namespace detail {
constexpr bool linear_topk16_selector_closed() {
  bool hit[3][2][2] = {};
  for (int d = 1; d <= 256; ++d)
    for (int dense = 0; dense < 2; ++dense)
      for (int dt = kBf16; dt <= kF16; ++dt) {
        const LinearTopk16Variant v = select_linear_topk16_variant(d, dense != 0, dt);
        if (!maxk::has_variant(kLinearTopk16Variants, v)) return false;
        if (v.dp < d || v.dp % 64 != 0 || v.dp > 256 || (v.dp > 64 && v.dp / 2 >= d)) return false;
        if (2 * lds_bytes(v.dp) > 160 * 1024 || lds_bytes(v.dp) > 64 * 1024) return false;
        if ((kTileRows + v.dp) % kLoadRows != 0 || kTileRows % kLoadRows != 0) return false;
        hit[v.dp == 64 ? 0 : v.dp == 128 ? 1 : 2][dense][dt - kBf16] = true;
      }
  for (auto& h : hit)
    for (auto& g : h)
      if (!g[0] || !g[1]) return false;
  return true;
}
}  // namespace detail
static_assert(detail::linear_topk16_selector_closed(),
              "the linear-topk16 selector leaves its table, or a table entry is never selected");

}  // namespace maxk_lt16
