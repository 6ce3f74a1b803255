// Holds the dispatch rules of csrc/variants.h to its tables, on the host (tooling, not product):
//
//   c++ -std=c++17 -Ispgemm-gnn_amd/csrc tools/variant_check.cpp -o variant_check
//
// For every kernel family it walks the selector's whole input domain and checks that each
// selected variant is in the family's table (or is the forward's documented refusal, 4-byte edge
// words on a shape without them) and that every table entry is selected by some input, so no
// instantiation is dead. It prints the tables' kernel names, sorted, one per line, as
// tests/golden/kernel_instantiations.txt lists them; problems go to stderr and exit status 1.
//
//   variant_check transpose
//
// does the same for the tables of csrc/variants_transpose.h alone (the transposition's passes over
// every pass count, and its digit plan over every key width); their names are the pass kernels of
// tests/golden/kernel_instantiations_transpose.txt.
//
//   variant_check linear
//
// does it for the tables of csrc/variants_linear.h (the panel kernels of the CBSR-times-table
// products over every D and the widths of M around the panel edges, with the panel cover and the
// scratch sizes); their names are the panel kernels of
// tests/golden/kernel_instantiations_linear.txt.
//
//   variant_check linear_topk
//
// does it for the table of csrc/variants_linear_topk.h (the fused linear + top-k kernel over every
// D, with and without the dense row, and its LDS plan); its names are
// tests/golden/kernel_instantiations_linear_topk.txt.
//
//   variant_check linear_topk16
//
// does it for the table of csrc/variants_linear_topk16.h (the 16-bit fused kernel over every D,
// with and without the dense row, for bf16 and f16, and its LDS plan); its names are
// tests/golden/kernel_instantiations_linear_topk16.txt.
//
//   variant_check weight_grad16
//
// does it for the table of csrc/variants_weight_grad16.h (the 16-bit weight gradient over every D,
// the widths of M around the panel edges and both types, with its wave tiling, LDS plan, row
// groups, scratch sizes and depth positions); its names are
// tests/golden/kernel_instantiations_weight_grad16.txt.
//
//   variant_check matmul16
//
// does it for the table of csrc/variants_matmul16.h (the 16-bit CBSR product over every D, the
// widths of M around the panel edges and both types, with its LDS plan, row groups and the two
// placements); its names are tests/golden/kernel_instantiations_matmul16.txt.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "variants.h"
#include "variants_linear.h"
#include "variants_linear_topk.h"
#include "variants_linear_topk16.h"
#include "variants_matmul16.h"
#include "variants_transpose.h"
#include "variants_weight_grad16.h"

using namespace maxk;

static int g_bad = 0;
static std::vector<std::string> g_names;

// One family: `seen[i]` counts the inputs that selected table[i].
template <class Table>
struct Family {
  const char* name;
  const Table& table;
  std::vector<long> seen;
  long inputs = 0, refused = 0;
  Family(const char* n, const Table& t) : name(n), table(t), seen(t.size(), 0) {}
  template <class V>
  void selected(const V& v) {
    ++inputs;
    for (size_t i = 0; i < table.size(); ++i)
      if (table[i] == v) {
        ++seen[i];
        return;
      }
    std::fprintf(stderr, "%s: selected %s, which is not in the table\n", name,
                 kernel_name(v).c_str());
    g_bad = 1;
  }
  ~Family() {
    for (size_t i = 0; i < table.size(); ++i) {
      g_names.push_back(kernel_name(table[i]));
      for (size_t j = 0; j < i; ++j)
        if (table[j] == table[i]) {
          std::fprintf(stderr, "%s: %s is listed twice\n", name, g_names.back().c_str());
          g_bad = 1;
        }
      if (seen[i] == 0) {
        std::fprintf(stderr, "%s: no input selects %s\n", name, g_names.back().c_str());
        g_bad = 1;
      }
    }
    std::fprintf(stderr, "%-12s %2zu variants, %6ld inputs, %5ld refused\n", name, table.size(),
                 inputs, refused);
  }
};

static int finish() {
  std::sort(g_names.begin(), g_names.end());
  for (const std::string& n : g_names) std::puts(n.c_str());
  return g_bad;
}

// The tables of variants_transpose.h: every pass of every pass count, with and without values;
// and the digit plan of every key width: widths within the limit that sum to the key's bits.
static int check_transpose() {
  using namespace maxk_tr;
  const bool tf[] = {false, true};
  {
    Family pass("tr_pass", kPassVariants);
    Family hist("tr_hist", kHistVariants);
    for (int passes = 1; passes <= kTrMaxPasses; ++passes)
      for (int p = 0; p < passes; ++p) {
        for (bool val : tf) pass.selected(select_pass_variant(p, passes, val));
        hist.selected(select_hist_variant(p));
      }
  }
  for (int b = 0; b <= 31; ++b)
    for (long long nc : {(1ll << b) - 1, 1ll << b, (1ll << b) + 1}) {
      if (nc > INT32_MAX) continue;
      const int32_t n = (int32_t)nc;
      const int passes = pass_count(n);
      int sum = 0, widest = 0;
      bool ok = passes >= 1 && passes <= kTrMaxPasses;
      for (int p = 0; p < passes; ++p) {
        const int w = digit_bits(n, p);
        ok = ok && digit_shift(n, p) == sum;
        sum += w;
        widest = w > widest ? w : widest;
      }
      if (!ok || sum != key_bits(n) || widest > kTrMaxDigitBits || (1ll << sum) < nc) {
        std::fprintf(stderr, "transpose: bad digit plan for %lld columns\n", nc);
        g_bad = 1;
      }
    }
  return finish();
}

// The tables of variants_linear.h: every D, and M up to past three wide panels; the panels cover M
// without an empty one, the row groups stay within kLinGroups over all panels, and the scratch
// sizes are the documented ones.
static int check_linear() {
  using namespace maxk_lin;
  {
    Family a("lin_matmul", kMatmulVariants);
    Family b("lin_sampled", kSampledVariants);
    Family c("lin_wgrad", kWeightGradVariants);
    for (int d = 1; d <= 256; ++d)
      for (int m = 1; m <= 400; ++m) {
        a.selected(select_matmul_variant(d, m));
        b.selected(select_sampled_variant(d, m));
        c.selected(select_weight_grad_variant(d, m));
        const int mp = panel_width(d, m);
        const long long p = panel_count(d, m);
        bool ok = (mp == 64 || mp == 128) && p * mp >= m && (p - 1) * mp < m &&
                  4ll * (d * mp + d) <= 160 * 1024;
        for (long long n : {0ll, 1ll, 16ll, 17ll, 4096ll, 4097ll, 232965ll, 2449029ll}) {
          const long long w = row_groups(n, p);
          ok = ok && w >= 1 && w * p <= (p > kLinGroups ? p : kLinGroups) &&
               (w - 1) * kLinWaves < (n > 0 ? n : 1) &&
               scratch_bytes(kLinMatmul, n, d, 1, m) == 0 &&
               scratch_bytes(kLinSampled, n, d, d, m) == (p > 1 ? 4 * p * n * d : 0) &&
               scratch_bytes(kLinWeightGrad, n, d, 1, m) == 4 * (p * w * d * mp + w * d);
        }
        if (!ok) {
          std::fprintf(stderr, "linear: bad panel plan for D = %d, M = %d\n", d, m);
          g_bad = 1;
        }
      }
  }
  if (scratch_bytes(3, 1, 8, 1, 1) != -1 || scratch_bytes(0, 1, 8, 9, 1) != -1 ||
      scratch_bytes(0, 1, 257, 1, 1) != -1 || scratch_bytes(0, 1, 8, 1, 0) != -1 ||
      scratch_bytes(0, -1, 8, 1, 1) != -1) {
    std::fprintf(stderr, "linear: scratch_bytes accepts a shape outside the limits\n");
    g_bad = 1;
  }
  return finish();
}

// The table of variants_linear_topk.h: every D with and without the dense row; the accumulators
// cover D with the narrowest width, and the stage and the waves' epilogue rows fit the LDS twice.
static int check_linear_topk() {
  using namespace maxk_lt;
  {
    Family fam("linear_topk", kLinearTopkVariants);
    for (int d = 1; d <= 256; ++d)
      for (bool dense : {false, true}) {
        const LinearTopkVariant v = select_linear_topk_variant(d, dense);
        fam.selected(v);
        const int dp = padded_dim(d);
        const bool ok = v.dp == dp && v.dense == dense && dp >= d && (dp == 64 || dp / 2 < d) &&
                        lds_bytes(dp) >= stage_bytes(dp) &&
                        lds_bytes(dp) >= kLtWaves * wave_epilogue_bytes(dp) &&
                        wave_epilogue_bytes(dp) % 16 == 0 && 2 * lds_bytes(dp) <= 160 * 1024 &&
                        (kLtTileRows + dp) % 32 == 0;
        if (!ok) {
          std::fprintf(stderr, "linear_topk: bad tile plan for D = %d\n", d);
          g_bad = 1;
        }
      }
  }
  return finish();
}

// The table of variants_linear_topk16.h: every D with and without the dense row in both types; the
// accumulators cover D with the narrowest width, the rounds of 16-byte loads cover the stage's rows
// and a staged row is whole MFMA steps, and the stage and the waves' epilogue rows fit the LDS
// twice.
static int check_linear_topk16() {
  using namespace maxk_lt16;
  {
    Family fam("linear_topk16", kLinearTopk16Variants);
    for (int d = 1; d <= 256; ++d)
      for (bool dense : {false, true})
        for (int dt : {kBf16, kF16}) {
          const LinearTopk16Variant v = select_linear_topk16_variant(d, dense, dt);
          fam.selected(v);
          const int dp = padded_dim(d);
          const bool ok = v.dp == dp && v.dense == dense && v.dtype == dt && dp >= d &&
                          (dp == 64 || dp / 2 < d) && lds_bytes(dp) >= stage_bytes(dp) &&
                          lds_bytes(dp) >= kWaves * wave_epilogue_bytes(dp) &&
                          wave_epilogue_bytes(dp) % 16 == 0 && 2 * lds_bytes(dp) <= 160 * 1024 &&
                          (kTileRows + dp) % kLoadRows == 0 && kChunk % kStep == 0 &&
                          (2 * kRowElems) % 16 == 0;
          if (!ok) {
            std::fprintf(stderr, "linear_topk16: bad tile plan for D = %d\n", d);
            g_bad = 1;
          }
        }
  }
  return finish();
}

// The table of variants_weight_grad16.h: every D, M up to past three wide panels and both types; the
// panels cover M without an empty one, the 8 waves tile the [DP, MP] accumulator in whole 16 x 16
// tiles, two work-groups fit the LDS, the row groups stay within kGroups over all panels with no
// group left without a chunk, the scratch is the documented one, and the depth positions of a step
// are a permutation whose two halves are what one transposing read and one 16-byte read deliver.
static int check_weight_grad16() {
  using namespace maxk_wg16;
  {
    Family fam("weight_grad16", kWeightGrad16Variants);
    for (int d = 1; d <= 256; ++d)
      for (int m = 1; m <= 400; ++m)
        for (int dt : {kBf16, kF16}) {
          const WeightGrad16Variant v = select_weight_grad16_variant(d, m, dt);
          fam.selected(v);
          const int dp = padded_dim(d), mp = panel_width(m);
          const long long p = panel_count(m);
          const int wf = waves_along_features(dp), wc = kWaves / wf;
          bool ok = v.dp == dp && v.mp == mp && v.dtype == dt && dp >= d &&
                    (dp == 64 || dp / 2 < d) && (mp == 64 || mp == 128) && p * mp >= m &&
                    (p - 1) * mp < m && wf * wc == kWaves && (dp / 16) % wf == 0 &&
                    (mp / 16) % wc == 0 && 2 * lds_bytes(dp, mp) <= 160 * 1024 &&
                    (2 * (mp + kGPad)) % 16 == 0 && (2 * kARow) % 16 == 0 &&
                    kThreads % (mp / 8) == 0 && kChunkRows % (kThreads / (mp / 8)) == 0;
          for (long long n : {0ll, 1ll, 64ll, 65ll, 8192ll, 8193ll, 232965ll, 2449029ll}) {
            const long long w = row_groups(n, p), chunks = (n + kChunkRows - 1) / kChunkRows;
            ok = ok && w >= 1 && w * p <= (p > kGroups ? p : kGroups) &&
                 w <= (chunks > 0 ? chunks : 1) && w <= group_cap(p) &&
                 scratch_bytes(n, d, 1, m) == 4 * (p * w * d * mp + w * d);
          }
          if (!ok) {
            std::fprintf(stderr, "weight_grad16: bad tile plan for D = %d, M = %d\n", d, m);
            g_bad = 1;
          }
        }
  }
  unsigned seen = 0;
  for (int r = 0; r < kStep; ++r) {
    const int pos = depth_position(r), q = pos / 8, e = pos % 8;
    seen |= 1u << pos;
    // lane (i, q) holds positions 8 q + e: rows 4 q + e of the first read, 16 + 4 q + e - 4 of the second
    if (r != (e < 4 ? 4 * q + e : 16 + 4 * q + e - 4)) {
      std::fprintf(stderr, "weight_grad16: row %d sits at depth position %d\n", r, pos);
      g_bad = 1;
    }
  }
  if (seen != 0xffffffffu || scratch_bytes(1, 8, 9, 1) != -1 || scratch_bytes(1, 257, 1, 1) != -1 ||
      scratch_bytes(1, 8, 1, 0) != -1 || scratch_bytes(-1, 8, 1, 1) != -1 ||
      scratch_bytes(1, 8, 0, 1) != -1) {
    std::fprintf(stderr, "weight_grad16: depth positions or scratch limits are off\n");
    g_bad = 1;
  }
  return finish();
}

// The table of variants_matmul16.h: every D, M up to past three wide panels and both types; the
// panels cover M without an empty one, a wave's 16 rows times the panel are whole pairs of 16 x 16
// tiles, one work-group fits the LDS with every row 16-byte aligned, the row groups stay within
// kGroups over all panels with no group left without a tile, and the placements of features and
// columns are the permutations that the transposing read and the 8-column stores want.
static int check_matmul16() {
  using namespace maxk_mm16;
  {
    Family fam("matmul16", kMatmul16Variants);
    for (int d = 1; d <= 256; ++d)
      for (int m = 1; m <= 400; ++m)
        for (int dt : {kBf16, kF16}) {
          const Matmul16Variant v = select_matmul16_variant(d, m, dt);
          fam.selected(v);
          const int dp = padded_dim(d), mp = panel_width(m);
          const long long p = panel_count(m);
          bool ok = v.dp == dp && v.mp == mp && v.dtype == dt && dp >= d &&
                    (dp == 64 || dp / 2 < d) && (mp == 64 || mp == 128) && p * mp >= m &&
                    (p - 1) * mp < m && (mp / 16) % 2 == 0 && dp % kStep == 0 &&
                    lds_bytes(dp, mp) <= kCuLdsBytes && waves_per_simd(dp, mp) == 2 &&
                    (2 * (mp + kTPad)) % 16 == 0 && (2 * (dp + kAPad)) % 16 == 0 &&
                    kTileRows * kSlotLanes == kThreads;
          for (long long n : {0ll, 1ll, 128ll, 129ll, 32768ll, 32769ll, 232965ll, 2449029ll}) {
            const long long w = row_groups(n, p), tiles = (n + kTileRows - 1) / kTileRows;
            ok = ok && w >= 1 && w * p <= (p > kGroups ? p : kGroups) &&
                 w <= (tiles > 0 ? tiles : 1) && w <= group_cap(p);
          }
          if (!ok) {
            std::fprintf(stderr, "matmul16: bad tile plan for D = %d, M = %d\n", d, m);
            g_bad = 1;
          }
        }
  }
  for (int r = 0; r < kStep; ++r) {
    const int pos = depth_position(r), q = pos / 8, e = pos % 8;
    const int col = staged_column(r), h = col / 16, cq = col % 16 / 4, cr = col % 4;
    // lane (i, q) holds positions 8 q + e: features 4 q + e of the first read, 16 + 4 q + e - 4 of
    // the second; register cr of lane group cq in tile h is column 8 cq + 4 h + cr
    if (r != (e < 4 ? 4 * q + e : 16 + 4 * q + e - 4) || r != 8 * cq + 4 * h + cr) {
      std::fprintf(stderr, "matmul16: feature / column %d sits at %d / %d\n", r, pos, col);
      g_bad = 1;
    }
  }
  return finish();
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "transpose") == 0) return check_transpose();
  if (argc > 1 && std::strcmp(argv[1], "linear") == 0) return check_linear();
  if (argc > 1 && std::strcmp(argv[1], "linear_topk") == 0) return check_linear_topk();
  if (argc > 1 && std::strcmp(argv[1], "linear_topk16") == 0) return check_linear_topk16();
  if (argc > 1 && std::strcmp(argv[1], "weight_grad16") == 0) return check_weight_grad16();
  if (argc > 1 && std::strcmp(argv[1], "matmul16") == 0) return check_matmul16();
  const bool tf[] = {false, true};
  {
    Family fam("forward", kFwdVariants);
    for (int layout = 0; layout <= 4; ++layout)
      for (int k = 1; k <= 256; ++k)
        for (bool fixed : tf)
          for (bool quad : tf)
            for (int waves : {4, 8})
              for (int unroll : {4, 8})
                for (bool rc : tf) {
                  const FwdVariant v = select_fwd_variant(layout, k, fixed, quad, waves, unroll, rc);
                  if (rc && v == kFwdNoRowconst) {
                    ++fam.inputs;
                    ++fam.refused;
                    // the refusal is the shapes without a 4-byte kernel, and no other: those
                    // are the quad-shared kernels of a fixed-point plan of 8 sub-steps
                    const FwdVariant w =
                        select_fwd_variant(layout, k, fixed, quad, waves, unroll, false);
                    if ((w.fl & kFwdFlagQuad) && fixed && unroll == 8) {
                      std::fprintf(stderr, "forward: refused %s with 4-byte words\n",
                                   kernel_name(w).c_str());
                      g_bad = 1;
                    }
                  } else {
                    fam.selected(v);
                  }
                }
  }
  {
    Family fam("stats4", kStats4Variants);
    for (bool rec : tf)
      for (bool stats : tf)
        for (bool pairs : tf)
          fam.selected(select_stats4_variant(rec, stats, pairs));
  }
  {
    Family fam("pack", kPackVariants);
    for (bool chunk3 : tf) fam.selected(select_pack_variant(chunk3));
  }
  {
    Family fam("bwd", kBwdVariants);
    for (int f : {4, 2})
      for (int lanes = 0; lanes < 4; ++lanes)
        for (int waves : {8, 12, 16})
          for (int unroll : {8, 12, 16})
            for (bool big : tf) fam.selected(select_bwd_variant(f, lanes, waves, unroll, big));
  }
  {
    Family fam("rows", kRowsVariants);
    for (int r : {1, 2, 4}) fam.selected(select_rows_variant(r));
  }
  {
    Family exact("topk_exact", kTopkExactVariants);
    Family ref("topk_ref", kTopkRefVariants);
    for (int d : {200, 256})
      for (int k : {16, 64, 65, 72})
        for (bool stats : tf)
          for (bool records : tf)
            for (bool drop : tf)
              for (bool dense : tf) {
                for (int n : {40, kTopkRows8 - 1, kTopkRows8})
                  exact.selected(select_topk_exact_variant(n, d, k, stats, records, drop, dense));
                ref.selected(select_topk_ref_variant(d, stats, records, drop, dense));
              }
  }
  {
    Family fam("scatter", kScatterVariants);
    for (bool drop : tf)
      for (bool merge : tf) fam.selected(select_scatter_variant(drop, merge));
  }
  {
    Family fam("sddmm", kSddmmVariants);
    for (int k = 1; k <= 256; ++k) fam.selected(select_sddmm_variant(k));
  }
  {
    Family fam("dense_spmm", kDenseSpmmVariants);
    for (int d = 4; d <= 1024; d += 4) fam.selected(select_dense_spmm_variant(d));
  }
  return finish();
}
