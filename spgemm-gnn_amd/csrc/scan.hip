// The plain exclusive scan (scan.h): the items are the values themselves.
#include "scan.h"

namespace maxk_scan {

struct PlainItem {
  static constexpr int kSums = 1;
  const int32_t* v;
  __device__ __forceinline__ void operator()(int64_t i, int32_t (&s)[1]) const { s[0] += v[i]; }
};

// v[0 .. n) becomes its exclusive scan, in place: a thread owns kItems consecutive items of its
// tile.
__global__ __launch_bounds__(kThreads) void apply_kernel(int32_t* v, int64_t n,
                                                         const int32_t* sums) {
  __shared__ int32_t red[kWaves];
  const int64_t first = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
  int32_t x[kItems], s = 0;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    x[q] = first + q < n ? v[first + q] : 0;
    s += x[q];
  }
  int32_t total;
  int32_t run = sums[blockIdx.x] + block_exclusive(s, red, total);
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    if (first + q < n) v[first + q] = run;
    run += x[q];
  }
}

void launch_apply(int32_t* v, int64_t n, const int32_t* sums, hipStream_t st) {
  hipLaunchKernelGGL(apply_kernel, dim3((unsigned)tiles(n)), dim3(kThreads), 0, st, v, n, sums);
}

void exclusive_scan(int32_t* v, int64_t n, int32_t* sums, hipStream_t st) {
  launch_tile_sums(PlainItem{v}, n, sums, st);
  launch_partials<1>(sums, tiles(n), nullptr, st);
  launch_apply(v, n, sums, st);
}

}  // namespace maxk_scan
