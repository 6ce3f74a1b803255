// Which kernel instantiation a launch runs, as data: for every templated kernel family the
// template arguments (a POD), the compiled set (a table, written once) and the rule that picks
// the variant from what the launcher knows (select_*). Plain C++17 with no HIP and no plan:
// the launchers dispatch over the tables (dispatch_variant, common.h), so the tables are the
// instantiations, and tools/variant_check.cpp holds the rules to the tables on the host.
#pragma once

#include <array>
#include <cstddef>
#include <string>
#include <utility>

namespace maxk {

constexpr int kWave = 64;               // CDNA wavefront width (never 32)
constexpr int kFwdThreads = 256;        // 4 waves per forward work-group
constexpr int kFwdUnroll = 8;           // independent sub-steps in flight per wave
constexpr int kFwdFlagChunk3 = 1;       // forward kernel flags (template FL): lane-chunk records
constexpr int kFwdFlagQuad = 2;         // quad-shared edge-word loads
constexpr int kFwdFlagChunk2 = 4;       // pair-chunk records: 2 values + their selectors per 16 B
// Rows whose loads a top-k wave issues up front: 8 on large inputs (ogbn-products 0.672 -> 0.647
// ms), 4 below kTopkRows8 rows, where the halved grid leaves a tail (Reddit 0.067 vs 0.071 ms).
constexpr int kTopkRows8 = 1 << 20;

namespace variants_detail {
inline std::string arg(int v) { return std::to_string(v); }
inline std::string arg(bool v) { return v ? "true" : "false"; }
// ns::kernel<a, ...> as the compiler's demangled name spells it
template <class... A>
std::string name_in(const char* ns, const char* kernel, A... a) {
  std::string s = std::string(ns) + "::" + kernel + "<", sep;
  ((s += sep + arg(a), sep = ", "), ...);
  return s + ">";
}
template <class... A>
std::string name(const char* kernel, A... a) {
  return name_in("maxk", kernel, a...);
}
}  // namespace variants_detail

// Whether `v` is one of the table's variants.
template <class Table, class V>
constexpr bool has_variant(const Table& table, const V& v) {
  for (const V& t : table)
    if (t == v) return true;
  return false;
}

// ---------------------------------------------------------------------------- forward
// spgemm_fwd_kernel<VEC, FL, NT, FU, RC>
struct FwdVariant {
  int v, fl, nt, fu;
  bool rc;
  constexpr bool operator==(const FwdVariant& o) const {
    return v == o.v && fl == o.fl && nt == o.nt && fu == o.fu && rc == o.rc;
  }
};
inline std::string kernel_name(const FwdVariant& x) {
  return variants_detail::name("spgemm_fwd_kernel", x.v, x.fl, x.nt, x.fu, x.rc);
}

// 7 (VEC, FL) x {8 waves x 8, 8 waves x 4, 4 waves x 8} with 8-byte edge words; the quad-shared
// FL x {8 waves, 4 waves} x 8 sub-steps with 4-byte words
inline constexpr std::array<FwdVariant, 27> kFwdVariants = [] {
  constexpr int vf[7][2] = {{1, 0},
                            {4, 0},
                            {4, kFwdFlagChunk3},
                            {4, kFwdFlagQuad},
                            {4, kFwdFlagChunk3 | kFwdFlagQuad},
                            {4, kFwdFlagChunk2},
                            {4, kFwdFlagChunk2 | kFwdFlagQuad}};
  std::array<FwdVariant, 27> t{};
  int n = 0;
  for (const auto& x : vf) {
    t[n++] = {x[0], x[1], 8 * kWave, kFwdUnroll, false};
    t[n++] = {x[0], x[1], 8 * kWave, 4, false};
    t[n++] = {x[0], x[1], kFwdThreads, kFwdUnroll, false};
    if (x[1] & kFwdFlagQuad) {
      t[n++] = {x[0], x[1], 8 * kWave, kFwdUnroll, true};
      t[n++] = {x[0], x[1], kFwdThreads, kFwdUnroll, true};
    }
  }
  return t;
}();

// select_fwd_variant's answer to 4-byte edge words on a shape that has no such kernel
inline constexpr FwdVariant kFwdNoRowconst = {0, 0, 0, 0, true};

// layout: maxk_plan_info.fwd_layout (2 lane chunks, 4 pair chunks, else values and selectors of
// the k slots as they are); fixed: the fixed-point forward; quad: the plan asks for quad-shared
// edge words; waves 4 or 8, unroll 4 or 8; rowconst: 4-byte edge words.
constexpr FwdVariant select_fwd_variant(int layout, int k, bool fixed, bool quad, int waves,
                                        int unroll, bool rowconst) {
  const bool chunk3 = layout == 2, chunk2 = layout == 4;
  const bool vec4 = k % 4 == 0 || chunk3 || chunk2;  // else one feature per lane, no flags
  const int lanes = chunk3 ? (k + 2) / 3 : chunk2 ? k / 2 : k / 4;  // lanes per edge
  const int fl = !vec4 ? 0
                       : (chunk3 ? kFwdFlagChunk3 : 0) | (chunk2 ? kFwdFlagChunk2 : 0) |
                             (quad && lanes % 4 == 0 ? kFwdFlagQuad : 0);
  const int nt = waves == 8 ? 8 * kWave : kFwdThreads;
  if (rowconst) {
    // 4-byte edge words: the quad kernels of 8 sub-steps of the fixed-point forward only
    if (!((fl & kFwdFlagQuad) && unroll == kFwdUnroll && fixed)) return kFwdNoRowconst;
    return {4, fl, nt, kFwdUnroll, true};
  }
  // 4 sub-steps only with 8 waves
  return {vec4 ? 4 : 1, fl, nt, waves == 8 && unroll == 4 ? 4 : kFwdUnroll, false};
}

// ---------------------------------------------------------------------------- statistics / pack
// cbsr_stats4_kernel<PACK, STATS>: PACK 2 pair chunks, 1 packed records, 0 none
struct Stats4Variant {
  int pack;
  bool stats;
  constexpr bool operator==(const Stats4Variant& o) const {
    return pack == o.pack && stats == o.stats;
  }
};
inline std::string kernel_name(const Stats4Variant& x) {
  return variants_detail::name("cbsr_stats4_kernel", x.pack, x.stats);
}
inline constexpr std::array<Stats4Variant, 5> kStats4Variants = {
    {{2, true}, {2, false}, {1, true}, {1, false}, {0, true}}};

// rec: the pass packs the forward's records; stats: it writes the statistics pair; pairs: the
// records are pair chunks. Without records it is the statistics pass.
constexpr Stats4Variant select_stats4_variant(bool rec, bool stats, bool pairs) {
  if (!rec) return {0, true};
  return {pairs ? 2 : 1, stats};
}

// pack_cbsr3_kernel<V>: V values and their selectors per 16-B chunk
struct PackVariant {
  int v;
  constexpr bool operator==(const PackVariant& o) const { return v == o.v; }
};
inline std::string kernel_name(const PackVariant& x) {
  return variants_detail::name("pack_cbsr3_kernel", x.v);
}
inline constexpr std::array<PackVariant, 2> kPackVariants = {{{3}, {2}}};
constexpr PackVariant select_pack_variant(bool chunk3) { return {chunk3 ? 3 : 2}; }

// ---------------------------------------------------------------------------- backward
// sspmm_bwd4_kernel<U, NT, F, Q, BIG>
struct BwdVariant {
  int u, nt, f;
  bool q, big;
  constexpr bool operator==(const BwdVariant& o) const {
    return u == o.u && nt == o.nt && f == o.f && q == o.q && big == o.big;
  }
};
inline std::string kernel_name(const BwdVariant& x) {
  return variants_detail::name("sspmm_bwd4_kernel", x.u, x.nt, x.f, x.q, x.big);
}

// 7 shapes {U, threads, BIG} x F {4, 2} x Q {true, false}
inline constexpr std::array<BwdVariant, 28> kBwdVariants = [] {
  constexpr int shapes[7][3] = {{8, 1024, 0},                           // 16 waves
                                {12, 768, 0}, {8, 768, 0},              // 12 waves
                                {16, 512, 0}, {12, 512, 0}, {8, 512, 0},  // 8 waves
                                {8, 512, 1}};                           // grad_out above 4 GiB
  std::array<BwdVariant, 28> t{};
  int n = 0;
  for (const auto& s : shapes)
    for (int f : {4, 2})
      for (bool q : {true, false}) t[n++] = {s[0], s[1], f, q, s[2] != 0};
  return t;
}();

// feats: selector slots per lane (4, else 2); lanes: lanes of an edge; waves / unroll: the
// plan's; big: grad_out exceeds 32-bit byte offsets.
constexpr BwdVariant select_bwd_variant(int feats, int lanes, int waves, int unroll, bool big) {
  const int f = feats == 4 ? 4 : 2;
  const bool q = lanes % 4 == 0;  // quad-aligned lane groups: batched record loads
  if (big) return {8, 8 * kWave, f, q, true};      // 64-bit gathers: one shape, 8 waves x 8
  if (waves == 16) return {8, 16 * kWave, f, q, false};  // 16 waves run U = 8
  if (waves == 12) return {unroll == 12 ? 12 : 8, 12 * kWave, f, q, false};  // U = 8 or 12
  return {unroll == 16 ? 16 : unroll == 12 ? 12 : 8, 8 * kWave, f, q, false};
}

// sspmm_bwd_rows_kernel<U, R>: R destination rows per wavefront
struct RowsVariant {
  int u, r;
  constexpr bool operator==(const RowsVariant& o) const { return u == o.u && r == o.r; }
};
inline std::string kernel_name(const RowsVariant& x) {
  return variants_detail::name("sspmm_bwd_rows_kernel", x.u, x.r);
}
inline constexpr std::array<RowsVariant, 3> kRowsVariants = {{{4, 4}, {4, 2}, {4, 1}}};
constexpr RowsVariant select_rows_variant(int rows_per_wave) {
  return {4, rows_per_wave == 4 ? 4 : rows_per_wave == 2 ? 2 : 1};
}

// ---------------------------------------------------------------------------- top-k, scatter
// topk_exact_kernel<kRowsPerWave, kWide, kFullRow, kStats, kRec, kDrop, kDense>
struct TopkExactVariant {
  int rows;
  bool wide, full, stats, rec, drop, dense;
  constexpr bool operator==(const TopkExactVariant& o) const {
    return rows == o.rows && wide == o.wide && full == o.full && stats == o.stats &&
           rec == o.rec && drop == o.drop && dense == o.dense;
  }
};
inline std::string kernel_name(const TopkExactVariant& x) {
  return variants_detail::name("topk_exact_kernel", x.rows, x.wide, x.full, x.stats, x.rec,
                               x.drop, x.dense);
}

// {rec, drop, dense} of the five kernel classes, in both top-k modes: plain, records, dropout,
// dense, dense with dropout (the dropout and dense kernels are record kernels)
inline constexpr bool kTopkClasses[5][3] = {{false, false, false},
                                            {true, false, false},
                                            {true, true, false},
                                            {true, false, true},
                                            {true, true, true}};

// 4 rows per wave: 5 classes x kWide x kFullRow x kStats, less the two dense kernels of a
// partial row of k <= 64 with statistics; 8 rows per wave: the plain kernel of k <= 64
inline constexpr std::array<TopkExactVariant, 40> kTopkExactVariants = [] {
  std::array<TopkExactVariant, 40> t{};
  int n = 0;
  for (const auto& c : kTopkClasses)
    for (bool wide : {false, true})
      for (bool full : {false, true})
        for (bool stats : {false, true})
          if (!(c[2] && !wide && !full && stats)) t[n++] = {4, wide, full, stats, c[0], c[1], c[2]};
  for (bool full : {false, true}) t[n++] = {8, false, full, false, false, false, false};
  return t;
}();

constexpr TopkExactVariant select_topk_exact_variant(int n, int d, int k, bool stats, bool records,
                                                     bool drop, bool dense) {
  const bool wide = k > kWave, full = d == 4 * kWave;
  // a dense partial row with statistics takes the k > 64 kernel at every k (its store loops run
  // once for k <= 64, same outputs): the k <= 64 one spills 4-7 VGPRs under the 64 cap
  if (dense) return {4, wide || (!full && stats), full, stats, true, drop, true};
  if (drop) return {4, wide, full, stats, true, true, false};
  // the statistics and record variants keep 4 rows per wave (with 8, 4-5 VGPRs spill under the
  // 64 cap with the statistics, 7-11 with the record store)
  if (!(wide || n < kTopkRows8 || stats || records))
    return {8, false, full, false, false, false, false};
  return {4, wide, full, stats, records, false, false};
}

// topk_ref_compat_kernel<kFullRow, kStats, kRec, kDrop, kDense>
struct TopkRefVariant {
  bool full, stats, rec, drop, dense;
  constexpr bool operator==(const TopkRefVariant& o) const {
    return full == o.full && stats == o.stats && rec == o.rec && drop == o.drop &&
           dense == o.dense;
  }
};
inline std::string kernel_name(const TopkRefVariant& x) {
  return variants_detail::name("topk_ref_compat_kernel", x.full, x.stats, x.rec, x.drop, x.dense);
}

// 5 classes x kFullRow x kStats
inline constexpr std::array<TopkRefVariant, 20> kTopkRefVariants = [] {
  std::array<TopkRefVariant, 20> t{};
  int n = 0;
  for (const auto& c : kTopkClasses)
    for (bool full : {false, true})
      for (bool stats : {false, true}) t[n++] = {full, stats, c[0], c[1], c[2]};
  return t;
}();

constexpr TopkRefVariant select_topk_ref_variant(int d, bool stats, bool records, bool drop,
                                                 bool dense) {
  return {d == 4 * kWave, stats, records || drop || dense, drop, dense};
}

// maxk_scatter_backward_kernel<kDrop, kMerge>
struct ScatterVariant {
  bool drop, merge;
  constexpr bool operator==(const ScatterVariant& o) const {
    return drop == o.drop && merge == o.merge;
  }
};
inline std::string kernel_name(const ScatterVariant& x) {
  return variants_detail::name("maxk_scatter_backward_kernel", x.drop, x.merge);
}
inline constexpr std::array<ScatterVariant, 4> kScatterVariants = {
    {{true, true}, {false, true}, {true, false}, {false, false}}};
constexpr ScatterVariant select_scatter_variant(bool drop, bool merge) { return {drop, merge}; }

// ---------------------------------------------------------------------------- SDDMM, dense SpMM
// sddmm_edge_grad_kernel<LP>: LP lanes per edge
struct SddmmVariant {
  int lanes;
  constexpr bool operator==(const SddmmVariant& o) const { return lanes == o.lanes; }
};
inline std::string kernel_name(const SddmmVariant& x) {
  return variants_detail::name("sddmm_edge_grad_kernel", x.lanes);
}
inline constexpr std::array<SddmmVariant, 7> kSddmmVariants = {
    {{1}, {2}, {4}, {8}, {16}, {32}, {64}}};

// k rounded up to a power of two: the slots an edge's lanes cover
constexpr int sddmm_slots(int k) {
  int k2 = 1;
  while (k2 < k) k2 <<= 1;
  return k2;
}
constexpr SddmmVariant select_sddmm_variant(int k) {
  const int k2 = sddmm_slots(k);
  return {k2 >= 4 ? k2 / 4 : 1};  // 4 slots per lane
}

// dense_spmm_kernel<L, U>: L lanes per row
struct DenseSpmmVariant {
  int l, u;
  constexpr bool operator==(const DenseSpmmVariant& o) const { return l == o.l && u == o.u; }
};
inline std::string kernel_name(const DenseSpmmVariant& x) {
  return variants_detail::name("dense_spmm_kernel", x.l, x.u);
}
inline constexpr std::array<DenseSpmmVariant, 5> kDenseSpmmVariants = {
    {{64, 4}, {32, 4}, {16, 4}, {8, 4}, {4, 4}}};
constexpr DenseSpmmVariant select_dense_spmm_variant(int d) {
  const int c4 = d / 4;  // float4 columns of a row
  return {c4 > 32 ? 64 : c4 > 16 ? 32 : c4 > 8 ? 16 : c4 > 4 ? 8 : 4, 4};
}

}  // namespace maxk
