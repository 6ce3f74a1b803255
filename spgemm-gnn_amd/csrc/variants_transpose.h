// The kernel instantiations of the CSR transposition (csrc/transpose.hip, namespace maxk_tr), as
// data, under the rule of variants.h: the template arguments are a POD, the compiled set is one
// constexpr table per kernel family, one select_* picks the variant, and the launcher dispatches
// over the table (dispatch_variant, common.h). The digit plan of the radix sort lives here too,
// because the entry points, tools/variant_check.cpp and the tests' restatement share it. Plain
// C++17 with no HIP.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

namespace maxk_tr {

constexpr int kTrWave = 64;
constexpr int kTrThreads = 256;                  // 4 waves per work-group
constexpr int kTrWaves = kTrThreads / kTrWave;
// A work-group owns a tile of kTrTile consecutive items of the pass's input order; wave w of it
// owns the sub-run [w * kTrSubRun, (w + 1) * kTrSubRun) of the tile and walks it 64 items at a
// time, kTrRounds times.
constexpr int kTrRounds = 32;
constexpr int kTrSubRun = kTrRounds * kTrWave;   // 2,048 items of a wave
constexpr int kTrTile = kTrWaves * kTrSubRun;    // 8,192 items of a work-group
// The widest digit: 2^11 counters of 4 B per wave, 32 KB of LDS per work-group.
constexpr int kTrMaxDigitBits = 11;
constexpr int kTrMaxDigits = 1 << kTrMaxDigitBits;
constexpr int kTrMaxPasses = 3;                  // 31 key bits in digits of at most 11

// Bits of the sort key: columns are in [0, num_cols), so bits(num_cols - 1); 0 for one column.
constexpr int key_bits(int32_t num_cols) {
  int b = 0;
  for (int64_t top = (int64_t)num_cols - 1; top > 0; top >>= 1) ++b;
  return b;
}
// The passes of the sort: ceil(key bits / kTrMaxDigitBits), at least one (a single column is one
// pass over a digit of no bits, which keeps the input order).
constexpr int pass_count(int32_t num_cols) {
  const int b = key_bits(num_cols);
  return b == 0 ? 1 : (b + kTrMaxDigitBits - 1) / kTrMaxDigitBits;
}
// Width of the digit of pass `pass` (the lowest digit is pass 0): the key bits split evenly, the
// lower passes one bit wider where the split leaves a remainder.
constexpr int digit_bits(int32_t num_cols, int pass) {
  const int b = key_bits(num_cols), p = pass_count(num_cols);
  return b / p + (pass < b % p ? 1 : 0);
}
constexpr int digit_shift(int32_t num_cols, int pass) {
  int s = 0;
  for (int i = 0; i < pass; ++i) s += digit_bits(num_cols, i);
  return s;
}

// scatter_pass_kernel<ROLE, VAL>. ROLE says what the pass reads and writes: the first pass reads
// idx (the edge number is the position) and writes (column, edge) pairs, a middle pass moves pairs,
// the last pass writes out_order / out_row (/ out_val, VAL) and a single pass does both ends.
enum : int { kTrFirst = 0, kTrMiddle = 1, kTrLast = 2, kTrOnly = 3 };
struct PassVariant {
  int role;
  bool val;
  constexpr bool operator==(const PassVariant& o) const {
    return role == o.role && val == o.val;
  }
};
inline std::string kernel_name(const PassVariant& x) {
  return "maxk_tr::scatter_pass_kernel<" + std::to_string(x.role) + ", " +
         (x.val ? "true" : "false") + ">";
}
inline constexpr std::array<PassVariant, 6> kPassVariants = {{
    {kTrFirst, false}, {kTrMiddle, false}, {kTrLast, false}, {kTrLast, true},
    {kTrOnly, false}, {kTrOnly, true}}};
constexpr PassVariant select_pass_variant(int pass, int passes, bool has_val) {
  const int role = passes == 1 ? kTrOnly
                   : pass == 0 ? kTrFirst
                   : pass == passes - 1 ? kTrLast : kTrMiddle;
  return {role, has_val && (role == kTrLast || role == kTrOnly)};
}

// tile_hist_kernel<FROM_IDX>: the digit counts of every tile, from idx (pass 0, which also counts
// the columns into out_ptr) or from the keys of the pass before.
struct HistVariant {
  bool from_idx;
  constexpr bool operator==(const HistVariant& o) const { return from_idx == o.from_idx; }
};
inline std::string kernel_name(const HistVariant& x) {
  return std::string("maxk_tr::tile_hist_kernel<") + (x.from_idx ? "true" : "false") + ">";
}
inline constexpr std::array<HistVariant, 2> kHistVariants = {{{false}, {true}}};
constexpr HistVariant select_hist_variant(int pass) { return {pass == 0}; }

// The selectors stay inside their tables over their whole domain, and every entry is selected by
// some input: checked where the tables are compiled.
namespace detail {
constexpr bool transpose_selectors_closed() {
  bool hit[kPassVariants.size()] = {};
  bool hist[kHistVariants.size()] = {};
  for (int passes = 1; passes <= kTrMaxPasses; ++passes)
    for (int pass = 0; pass < passes; ++pass) {
      for (bool v : {false, true}) {
        const PassVariant s = select_pass_variant(pass, passes, v);
        bool found = false;
        for (size_t i = 0; i < kPassVariants.size(); ++i)
          if (kPassVariants[i] == s) found = hit[i] = true;
        if (!found) return false;
      }
      const HistVariant h = select_hist_variant(pass);
      bool found = false;
      for (size_t i = 0; i < kHistVariants.size(); ++i)
        if (kHistVariants[i] == h) found = hist[i] = true;
      if (!found) return false;
    }
  for (bool b : hit)
    if (!b) return false;
  for (bool b : hist)
    if (!b) return false;
  return true;
}
}  // namespace detail
static_assert(detail::transpose_selectors_closed(),
              "a transpose selector leaves its table, or a table entry is never selected");
static_assert(pass_count(INT32_MAX) <= kTrMaxPasses && digit_bits(INT32_MAX, 0) <= kTrMaxDigitBits,
              "the digit plan exceeds its limits");

}  // namespace maxk_tr
