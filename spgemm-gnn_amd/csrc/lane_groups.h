// The shape that the plan-less aggregations share (heads_aggregate.hip, max_aggregate.hip): an
// edge is served by LP adjacent lanes (a lane group), LP = lanes(k); lane `sub` of the group
// holds slot sub (and sub + 64, ... above k = 64). A work-group of 4 waves owns a tile of kTile
// rows (columns, in a backward) and serves each by its length: at most kShortMax edges by one lane
// group, at most kMediumMax by one wave whose 64 / LP groups take the edges j = g, g + G, ..., a
// longer one by the whole work-group.
//
// Two parts. The geometry is plain C++17 with no HIP, for the variant tables (variants_heads.h,
// variants_max.h). The device and launcher helpers follow under __HIPCC__: a thread's place, the
// three passes over a tile, the backward's combination of the groups' partial sums, and the
// argument checks and grid that the entry points share. No kernel lives here.
#pragma once

#include "variants.h"

namespace maxk::lg {

constexpr int kThreads = 256;              // 4 waves per work-group
constexpr int kWaves = kThreads / kWave;
constexpr int kTile = 16;                  // rows (columns) of a work-group
constexpr int kMinLanes = 8;               // lanes of an edge, at least
constexpr int kShortMax = 16;
constexpr int kMediumMax = 512;

// k rounded up to a power of two within [kMinLanes, kWave]
constexpr int lanes(int k) {
  int lp = kMinLanes;
  while (lp < k && lp < kWave) lp <<= 1;
  return lp;
}

}  // namespace maxk::lg

#ifdef __HIPCC__
#include "common.h"

namespace maxk::lg {

static_assert(kWaves == 4, "the hub pass combines four waves");

// slots of a lane in a backward, which keeps them in registers
constexpr int lane_slots(int lp) { return lp == kWave ? kMaxDim / kWave : 1; }

// LDS accesses of one wave are executed in program order; this keeps the compiler from moving
// them across the point where lanes read what other lanes of the wave wrote.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A thread's place: lane group g of its wave (gid of the work-group), lane sub of the group.
// An aggregate: `const Place<LP> p{};` in a kernel evaluates the initialisers there.
template <int LP>
struct Place {
  static constexpr int G = kWave / LP;   // lane groups of a wave
  static constexpr int NG = kWaves * G;  // of the work-group
  int tid = threadIdx.x;
  int lane = tid & (kWave - 1), wave = tid / kWave;
  int g = lane / LP, sub = lane % LP, gid = wave * G + g;
};

// ------------------------------------------------------------------------------ the tile walk
// f(row, b, n) for the rows of the tile at row0 that the caller serves in each regime, [b, b + n)
// the row's clamped segment of ptr. short_rows and medium_rows start at the thread's group or
// wave and take its Place; hub_rows visits every row with every thread and needs none.
//
// ptr, num_rows and E are taken by const reference on purpose, bound to the fields of the
// kernel's argument struct, so that they are read where they are used, as in a loop written in
// the kernel. By value the forward kernels come out with other register counts
// (profiles/lane_groups.md, "Device code"): do not simplify the signatures without comparing the
// device code again (tools/kernel_code_diff.py).

// short rows (and empty ones): one lane group each
template <int LP, class F>
__device__ __forceinline__ void short_rows(const Place<LP> p, const int32_t* const& ptr,
                                           int64_t row0, const int32_t& num_rows,
                                           const int64_t& E, F&& f) {
  int64_t b;
  int32_t n;
  for (int t = p.gid; t < kTile; t += Place<LP>::NG) {
    const int64_t row = row0 + t;
    row_segment(ptr, row, num_rows, E, b, n);
    if (row >= num_rows || n > kShortMax) continue;
    f(row, b, n);
  }
}

// medium rows: one wave each (wave-uniform branch)
template <int LP, class F>
__device__ __forceinline__ void medium_rows(const Place<LP> p, const int32_t* const& ptr,
                                            int64_t row0, const int32_t& num_rows,
                                            const int64_t& E, F&& f) {
  int64_t b;
  int32_t n;
  for (int t = p.wave; t < kTile; t += kWaves) {
    const int64_t row = row0 + t;
    row_segment(ptr, row, num_rows, E, b, n);
    if (n <= kShortMax || n > kMediumMax) continue;
    f(row, b, n);
  }
}

// hub rows: the whole work-group. Every thread walks every row of the tile and takes the same
// branch, so f is entered by all threads or by none: f may hold __syncthreads().
template <class F>
__device__ __forceinline__ void hub_rows(const int32_t* const& ptr, int64_t row0,
                                         const int32_t& num_rows, const int64_t& E, F&& f) {
  int64_t b;
  int32_t n;
  for (int t = 0; t < kTile; ++t) {
    const int64_t row = row0 + t;
    row_segment(ptr, row, num_rows, E, b, n);
    if (n <= kMediumMax) continue;
    f(row, b, n);
  }
}

// ----------------------------------------------------------------- the backward's combination
// gsp[i]: a lane's partial sum of slot sub + LP i over the entries its group took, S =
// lane_slots(LP) of them. out: the [rows, k] table, row the one that was served.

// a short row: the group had every entry
template <int LP, int S>
__device__ __forceinline__ void store_group(const Place<LP> p, const float (&gsp)[S], int k,
                                            float* out, int64_t row) {
#pragma unroll
  for (int i = 0; i < S; ++i)
    if (p.sub + LP * i < k) out[row * k + p.sub + LP * i] = gsp[i];
}

// the groups of a wave by a butterfly, every lane ends with the wave's sum
template <int LP, int S>
__device__ __forceinline__ void reduce_wave(float (&gsp)[S], int i) {
#pragma unroll
  for (int m = LP; m < kWave; m <<= 1) gsp[i] = gsp[i] + __shfl_xor(gsp[i], m, kWave);
}

// a medium row: the wave's groups combined, stored by group 0
template <int LP, int S>
__device__ __forceinline__ void reduce_wave_and_store(const Place<LP> p, float (&gsp)[S], int k,
                                                      float* out, int64_t row) {
#pragma unroll
  for (int i = 0; i < S; ++i) {
    reduce_wave<LP>(gsp, i);
    if (p.g == 0 && p.sub + LP * i < k) out[row * k + p.sub + LP * i] = gsp[i];
  }
}

// a hub row: the waves' sums through red as (w0 + w1) + (w2 + w3). Two barriers: call it from
// the hub pass alone.
template <int LP, int S>
__device__ __forceinline__ void reduce_block_and_store(const Place<LP> p, float (&gsp)[S], int k,
                                                       float* out, int64_t row,
                                                       float (&red)[kWaves][kMaxDim]) {
  __syncthreads();  // red is free (the tile's previous hub was read)
#pragma unroll
  for (int i = 0; i < S; ++i) {
    reduce_wave<LP>(gsp, i);
    if (p.g == 0 && p.sub + LP * i < k) red[p.wave][p.sub + LP * i] = gsp[i];
  }
  __syncthreads();
  for (int l = p.tid; l < k; l += kThreads)
    out[row * k + l] = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
}

// ------------------------------------------------------------------------------- entry points
// Sizes, k and the selector stride that every call of both operators checks; index_stride is
// resolved (0: k). `more`: the operator's own checks, which come after k and before the stride.
template <class More>
int check_shape(const std::string& w, int32_t num_rows, int32_t num_cols, int64_t E, int32_t D,
                int32_t k, int64_t& is, More&& more) {
  MAXK_CHECK_ARG(num_rows >= 0 && num_cols >= 0 && E >= 0 && E <= (int64_t)INT32_MAX,
                 w + "sizes out of range");
  MAXK_CHECK_ARG(D >= 1 && D <= kMaxDim, w + "dim_origin must be in [1, 256]");
  MAXK_CHECK_ARG(k >= 1 && k <= D, w + "k must be between 1 and input dimension");
  if (int rc = more()) return rc;
  if (is == 0) is = k;
  MAXK_CHECK_ARG(is >= k, w + "index_stride must be >= k (0: k)");
  MAXK_CHECK_ARG(E == 0 || num_cols > 0, w + "sizes out of range: edges without columns");
  MAXK_CHECK_ARG(E == 0 || num_rows > 0, w + "sizes out of range: edges without rows");
  return MAXK_OK;
}

inline int check_shape(const std::string& w, int32_t num_rows, int32_t num_cols, int64_t E,
                       int32_t D, int32_t k, int64_t& is) {
  return check_shape(w, num_rows, num_cols, E, D, k, is, [] { return (int)MAXK_OK; });
}

// one work-group per tile of n rows (columns)
inline dim3 tile_grid(int32_t n) { return dim3((unsigned)(((int64_t)n + kTile - 1) / kTile)); }

}  // namespace maxk::lg
#endif  // __HIPCC__
