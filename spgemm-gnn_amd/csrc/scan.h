// The exclusive scan of the graph operators (sample.hip, subgraph.hip, transpose.hip): int32
// items, in place, as three launches on tiles of kTile items, in a fixed order, through
// caller-supplied scratch.
//
//   tile_sums_kernel<Item>  sums[b] = the sum of tile b's items. An Item may add up to three sums
//                           per item; array j of the tile sums lives at sums + j * nb
//   partials_kernel<SUMS>   one work-group: array 0 becomes its exclusive scan, and the total of
//                           array j goes to totals[j]. The side arrays are only reduced
//   apply_kernel            v becomes its exclusive scan on top of its tile's scanned sum
//
// The tile-sum kernel strides its tile by work-group (item q * kThreads + tid of the tile), the
// apply kernel gives each thread kItems consecutive items: a caller that places items itself
// behind the first two steps (sample.hip's compaction) owns its items the second way.
//
// The kernels of the plain case (the items are v itself, no side sums) live in scan.hip behind
// exclusive_scan and launch_apply; an Item of a caller's own is instantiated where it is defined.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace maxk_scan {

constexpr int kWave = 64;
constexpr int kThreads = 256;  // 4 waves per work-group
constexpr int kWaves = kThreads / kWave;
constexpr int kItems = 8;      // items of a thread
constexpr int kTile = kThreads * kItems;
static_assert(kWaves == 4, "the sums of the per-wave words name four waves");

__device__ __forceinline__ int32_t wave_sum(int32_t v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// Exclusive scan of the calling work-group's 256 values: returns the sum of the values of the
// threads below, and the total in `total`. red: kWaves words of LDS, free on entry and on return.
__device__ __forceinline__ int32_t block_exclusive(int32_t v, int32_t* red, int32_t& total) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  int32_t inc = v;
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const int32_t o = __shfl_up(inc, m, kWave);
    if (lane >= m) inc += o;
  }
  if (lane == kWave - 1) red[wave] = inc;
  __syncthreads();
  int32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int32_t x = red[w];
    before += w < wave ? x : 0;
    all += x;
  }
  total = all;
  __syncthreads();  // red is free again
  return before + inc - v;
}

// Item: a trivially copyable functor with `static constexpr int kSums` (1 to 3) and
//   __device__ void operator()(int64_t i, int32_t (&s)[kSums]) const
// which adds item i's contributions to the sums; it is called for 0 <= i < n.
template <class Item>
__global__ __launch_bounds__(kThreads) void tile_sums_kernel(const Item item, int64_t n,
                                                             int64_t nb, int32_t* sums) {
  constexpr int S = Item::kSums;
  static_assert(S >= 1 && S <= 3, "one to three sums per item");
  __shared__ int32_t red[S][kWaves];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  int32_t s[S] = {};
  for (int q = 0; q < kItems; ++q) {
    const int64_t i = base + (int64_t)q * kThreads + tid;
    if (i < n) item(i, s);
  }
#pragma unroll
  for (int j = 0; j < S; ++j) {
    s[j] = wave_sum(s[j]);
    if ((tid & (kWave - 1)) == 0) red[j][tid / kWave] = s[j];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < S; ++j)
      sums[j * nb + blockIdx.x] = (red[j][0] + red[j][1]) + (red[j][2] + red[j][3]);
  }
}

// One work-group over the SUMS arrays of nb tile sums: sums[0 .. nb) becomes its exclusive scan
// (256 at a time, the carry running across the rounds); with totals, totals[j] = the total of
// array j.
template <int SUMS>
__global__ __launch_bounds__(kThreads) void partials_kernel(int32_t* sums, int64_t nb,
                                                            int32_t* totals) {
  static_assert(SUMS >= 1 && SUMS <= 3, "one to three arrays of tile sums");
  constexpr int SIDE = SUMS - 1;
  __shared__ int32_t red[kWaves];
  __shared__ int32_t tot[SIDE > 0 ? SIDE : 1][kWaves];
  const int tid = threadIdx.x;
  int32_t carry = 0;
  int32_t side[SIDE > 0 ? SIDE : 1] = {};  // this thread's share of the side totals
  for (int64_t i0 = 0; i0 < nb; i0 += kThreads) {
    const int64_t i = i0 + tid;
    int32_t total;
    const int32_t ex = block_exclusive(i < nb ? sums[i] : 0, red, total);
    if (i < nb) {
      sums[i] = carry + ex;
#pragma unroll
      for (int j = 0; j < SIDE; ++j) side[j] += sums[(j + 1) * nb + i];
    }
    carry += total;
  }
  if constexpr (SIDE > 0) {
#pragma unroll
    for (int j = 0; j < SIDE; ++j) {
      side[j] = wave_sum(side[j]);
      if ((tid & (kWave - 1)) == 0) tot[j][tid / kWave] = side[j];
    }
    __syncthreads();
  }
  if (tid == 0 && totals) {
    totals[0] = carry;
#pragma unroll
    for (int j = 0; j < SIDE; ++j)
      totals[j + 1] = (tot[j][0] + tot[j][1]) + (tot[j][2] + tot[j][3]);
  }
}

// ------------------------------------------------------------------------------------- host
inline int64_t tiles(int64_t n) { return (n + kTile - 1) / kTile; }

// sums: tiles(n) words per sum of the Item
template <class Item>
void launch_tile_sums(const Item& item, int64_t n, int32_t* sums, hipStream_t st) {
  const int64_t nb = tiles(n);
  hipLaunchKernelGGL(tile_sums_kernel<Item>, dim3((unsigned)nb), dim3(kThreads), 0, st, item, n,
                     nb, sums);
}

// totals: SUMS words, or NULL
template <int SUMS>
void launch_partials(int32_t* sums, int64_t nb, int32_t* totals, hipStream_t st) {
  hipLaunchKernelGGL(partials_kernel<SUMS>, dim3(1), dim3(kThreads), 0, st, sums, nb, totals);
}

// v[0 .. n) becomes its exclusive scan on top of sums[tile], the scanned tile sums.
void launch_apply(int32_t* v, int64_t n, const int32_t* sums, hipStream_t st);

// v[0 .. n) becomes its exclusive scan, in place; sums: tiles(n) words of scratch.
void exclusive_scan(int32_t* v, int64_t n, int32_t* sums, hipStream_t st);

}  // namespace maxk_scan
