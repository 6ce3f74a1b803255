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
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "variants.h"
#include "variants_transpose.h"

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

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "transpose") == 0) return check_transpose();
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
