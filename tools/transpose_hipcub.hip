// Stand-alone comparator of the CSR transposition (tooling, not linked into the library):
// hipcub::DeviceRadixSort::SortPairs of (column, edge number) pairs over the key bits the library
// sorts, bits(num_cols - 1), on uniformly random columns. It is the sort alone: no out_ptr, no
// rows, no values.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/transpose_hipcub.hip -o tools/transpose_hipcub
//   tools/transpose_hipcub NUM_EDGES NUM_COLS [ROUNDS [REPS]]
//
// Prints one JSON line: the median and the extremes of ROUNDS windows of REPS sorts (HIP events).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <hipcub/hipcub.hpp>
#include <vector>

#define TRY(expr)                                                                  \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));              \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

__global__ void fill_kernel(int32_t* keys, int32_t* eids, int64_t n, uint32_t num_cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t x = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  keys[i] = (int32_t)((x >> 16) % num_cols);
  eids[i] = (int32_t)i;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s NUM_EDGES NUM_COLS [ROUNDS [REPS]]\n", argv[0]);
    return 2;
  }
  const int64_t n = std::atoll(argv[1]);
  const int64_t num_cols = std::atoll(argv[2]);
  const int rounds = argc > 3 ? std::atoi(argv[3]) : 7;
  const int reps = argc > 4 ? std::atoi(argv[4]) : 20;
  if (n <= 0 || n > INT32_MAX || num_cols <= 0 || num_cols > INT32_MAX || rounds < 1 || reps < 1) {
    std::fprintf(stderr, "sizes out of range\n");
    return 2;
  }
  int bits = 0;
  for (int64_t top = num_cols - 1; top > 0; top >>= 1) ++bits;
  const int end_bit = bits > 0 ? bits : 1;

  int32_t *keys_in, *keys_out, *eids_in, *eids_out;
  TRY(hipMalloc(&keys_in, 4 * n));
  TRY(hipMalloc(&keys_out, 4 * n));
  TRY(hipMalloc(&eids_in, 4 * n));
  TRY(hipMalloc(&eids_out, 4 * n));
  fill_kernel<<<(unsigned)((n + 255) / 256), 256>>>(keys_in, eids_in, n, (uint32_t)num_cols);
  TRY(hipGetLastError());
  size_t temp_bytes = 0;
  TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, keys_in, keys_out, eids_in, eids_out,
                                         (int)n, 0, end_bit));
  void* temp = nullptr;
  TRY(hipMalloc(&temp, temp_bytes));
  auto sort = [&]() {
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys_in, keys_out, eids_in,
                                              eids_out, (int)n, 0, end_bit);
  };
  TRY(sort());
  TRY(sort());
  TRY(hipDeviceSynchronize());
  hipEvent_t start, stop;
  TRY(hipEventCreate(&start));
  TRY(hipEventCreate(&stop));
  std::vector<float> ms;
  for (int r = 0; r < rounds; ++r) {
    TRY(hipEventRecord(start));
    for (int i = 0; i < reps; ++i) TRY(sort());
    TRY(hipEventRecord(stop));
    TRY(hipEventSynchronize(stop));
    float t = 0;
    TRY(hipEventElapsedTime(&t, start, stop));
    ms.push_back(t / reps);
  }
  std::sort(ms.begin(), ms.end());
  std::printf("{\"hipcub_edges\": %lld, \"hipcub_cols\": %lld, \"hipcub_key_bits\": %d, "
              "\"hipcub_temp_bytes\": %zu, \"hipcub_ms\": %.6f, \"hipcub_min_max_ms\": [%.6f, %.6f]}\n",
              (long long)n, (long long)num_cols, bits, temp_bytes, ms[ms.size() / 2], ms.front(),
              ms.back());
  return 0;
}
