// Softmax of per-edge logits over each destination row's in-edges, and its gradient
// (include/maxk_hip.h, "Edge softmax").
//
//   forward   m = max x_e,  p_e = expf(x_e - m),  s = sum p_e,  out_e = p_e * (1 / s)
//   backward  t = sum y_e * g_e,  grad_e = y_e * (g_e - t)
//
// A CSR row is one contiguous segment of ptr, so both are pure streaming kernels with a
// reduction per segment: no atomics, no scratch, no plan.
//
// Shape: one 256-thread work-group per tile of kEsTileRows consecutive rows; wave w of the
// group owns rows 4w .. 4w + 3 of the tile. A row is served by its length n alone:
//   * short,  n <= kEsShortMax (64): by 16 lanes (the four rows of a wave side by side), four
//     elements per lane in registers, 4-level xor butterflies;
//   * medium, n <= kEsMediumMax (1024): by its wave, S = 2, 4, 8 or 16 elements per lane in
//     registers (the smallest S with 64 S >= n), read once and written once;
//   * hub, above: by the whole work-group that owns its tile, every thread striding the segment
//     by 256, waves combined through LDS; the segment is read again per pass (two extra reads
//     forward, one backward) out of the L2, which a segment of this size has just filled.
// Hub rows reach a work-group with no list of them: every thread of the group reads the tile's
// row lengths, so the group agrees on its hubs and takes them together after its waves' own
// rows. A 20,000-edge hub is 80 KB, microseconds for one work-group, and the 16-row tiles of a
// graph outnumber the CUs by far, so the dispatcher levels the difference.
// Element j of a row always sits in lane j % W, slot j / W (W = 16, 64 or 256 by the row's
// length): a lane sums its slots in order, then the butterfly. Position, neighbours, the
// segment's alignment and num_rows never enter, so a row's bits depend on its values and length.
// Loads are one dword per lane, 64 contiguous lanes: vector loads would tie the order to
// ptr[r] % 4.
#include "common.h"

// every product, difference and sum below is one IEEE operation
#pragma clang fp contract(off)

namespace maxk {

constexpr int kEsThreads = 256;
constexpr int kEsWaves = kEsThreads / kWave;
constexpr int kEsGroup = 16;                           // lanes of a short row
constexpr int kEsWaveRows = kWave / kEsGroup;          // rows of a wave
constexpr int kEsTileRows = kEsWaves * kEsWaveRows;    // rows of a work-group
constexpr int kEsShortSlots = 4;
constexpr int kEsShortMax = kEsGroup * kEsShortSlots;  // 64
constexpr int kEsMediumSlots = 16;
constexpr int kEsMediumMax = kWave * kEsMediumSlots;   // 1024
constexpr int kEsHubUnroll = 4;

template <int W>
__device__ __forceinline__ float es_max(float v) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
  return v;
}

template <int W>
__device__ __forceinline__ float es_sum(float v) {
#pragma unroll
  for (int m = 1; m < W; m <<= 1) v = v + __shfl_xor(v, m, kWave);
  return v;
}

// Segment [b, b + n) of a row, clamped into [0, E] so that a ptr that breaks the documented
// preconditions still indexes inside the arrays.
__device__ __forceinline__ void es_segment(const int32_t* __restrict__ ptr, int64_t row,
                                           int32_t num_rows, int64_t E, int64_t& b, int32_t& n) {
  b = 0;
  n = 0;
  if (row < num_rows) {
    int64_t lo = ptr[row], hi = ptr[row + 1];
    lo = lo < 0 ? 0 : (lo > E ? E : lo);
    hi = hi < lo ? lo : (hi > E ? E : hi);
    b = lo;
    n = (int32_t)(hi - lo);
  }
}

// ---------------------------------------------------------------------------------- forward
// W lanes (lane `sub` of them) hold S slots each of the row x[0, n), n in [0, W * S]. Loads are
// unconditional at a clamped index (`safe`: an in-bounds element for a group with no row), so
// all S are in flight together.
template <int W, int S>
__device__ __forceinline__ void es_fwd_regs(const float* __restrict__ x, float* __restrict__ out,
                                            int32_t n, int sub) {
  float v[S];
  const int32_t last = n > 0 ? n - 1 : 0;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int32_t j = sub + W * i;
    v[i] = x[j < last ? j : last];
  }
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < S; ++i) m = fmaxf(m, sub + W * i < n ? v[i] : -INFINITY);
  m = es_max<W>(m);
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    v[i] = sub + W * i < n ? expf(v[i] - m) : 0.f;
    a = a + v[i];
  }
  const float inv = 1.0f / es_sum<W>(a);
#pragma unroll
  for (int i = 0; i < S; ++i)
    if (sub + W * i < n) out[sub + W * i] = v[i] * inv;
}

__global__ __launch_bounds__(kEsThreads) void edge_softmax_fwd_kernel(
    const int32_t* __restrict__ ptr, const float* __restrict__ logits, float* __restrict__ out,
    int32_t num_rows, int64_t E) {
  __shared__ float red[2 * kEsWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kEsTileRows;

  // the wave's own rows: short ones side by side, medium ones one after the other
  int64_t b;
  int32_t n;
  es_segment(ptr, row0 + wave * kEsWaveRows + lane / kEsGroup, num_rows, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  if (__ballot(ns > 0) != 0) {
    // a group with no short row reads element 0 (E > 0) and writes nothing
    const int64_t bs = ns > 0 ? b : 0;
    es_fwd_regs<kEsGroup, kEsShortSlots>(logits + bs, out + bs, ns, lane % kEsGroup);
  }
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    const float* x = logits + bg;
    float* o = out + bg;
    if (ng <= 2 * kWave) es_fwd_regs<kWave, 2>(x, o, ng, lane);
    else if (ng <= 4 * kWave) es_fwd_regs<kWave, 4>(x, o, ng, lane);
    else if (ng <= 8 * kWave) es_fwd_regs<kWave, 8>(x, o, ng, lane);
    else es_fwd_regs<kWave, kEsMediumSlots>(x, o, ng, lane);
  }

  // the tile's hub rows: every thread reads the same lengths, so the branch is group-uniform
  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    es_segment(ptr, row0 + r, num_rows, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    const float* x = logits + bh;
    float* o = out + bh;
    float m = -INFINITY;
#pragma unroll kEsHubUnroll
    for (int32_t j = tid; j < nh; j += kEsThreads) m = fmaxf(m, x[j]);
    m = es_max<kWave>(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float a = 0.f;
#pragma unroll kEsHubUnroll
    for (int32_t j = tid; j < nh; j += kEsThreads) a = a + expf(x[j] - m);
    a = es_sum<kWave>(a);
    if (lane == 0) red[kEsWaves + wave] = a;
    __syncthreads();
    const float inv = 1.0f / ((red[kEsWaves] + red[kEsWaves + 1]) +
                              (red[kEsWaves + 2] + red[kEsWaves + 3]));
#pragma unroll kEsHubUnroll
    for (int32_t j = tid; j < nh; j += kEsThreads) o[j] = expf(x[j] - m) * inv;
    __syncthreads();  // red is free for the tile's next hub
  }
}
static_assert(kEsWaves == 4, "the hub rows combine four waves");

// --------------------------------------------------------------------------------- backward
template <int W, int S>
__device__ __forceinline__ void es_bwd_regs(const float* __restrict__ y,
                                            const float* __restrict__ gy, float* __restrict__ out,
                                            int32_t n, int sub) {
  float v[S], g[S];
  const int32_t last = n > 0 ? n - 1 : 0;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int32_t j = sub + W * i;
    v[i] = y[j < last ? j : last];
    g[i] = gy[j < last ? j : last];
  }
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) a = a + (sub + W * i < n ? v[i] * g[i] : 0.f);
  const float t = es_sum<W>(a);
#pragma unroll
  for (int i = 0; i < S; ++i)
    if (sub + W * i < n) out[sub + W * i] = v[i] * (g[i] - t);
}

__global__ __launch_bounds__(kEsThreads) void edge_softmax_bwd_kernel(
    const int32_t* __restrict__ ptr, const float* __restrict__ y, const float* __restrict__ gy,
    float* __restrict__ out, int32_t num_rows, int64_t E) {
  __shared__ float red[kEsWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kEsTileRows;

  int64_t b;
  int32_t n;
  es_segment(ptr, row0 + wave * kEsWaveRows + lane / kEsGroup, num_rows, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  if (__ballot(ns > 0) != 0) {
    const int64_t bs = ns > 0 ? b : 0;
    es_bwd_regs<kEsGroup, kEsShortSlots>(y + bs, gy + bs, out + bs, ns, lane % kEsGroup);
  }
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    if (ng <= 2 * kWave) es_bwd_regs<kWave, 2>(y + bg, gy + bg, out + bg, ng, lane);
    else if (ng <= 4 * kWave) es_bwd_regs<kWave, 4>(y + bg, gy + bg, out + bg, ng, lane);
    else if (ng <= 8 * kWave) es_bwd_regs<kWave, 8>(y + bg, gy + bg, out + bg, ng, lane);
    else es_bwd_regs<kWave, kEsMediumSlots>(y + bg, gy + bg, out + bg, ng, lane);
  }

  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    es_segment(ptr, row0 + r, num_rows, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    const float* yv = y + bh;
    const float* gv = gy + bh;
    float* o = out + bh;
    float a = 0.f;
#pragma unroll kEsHubUnroll
    for (int32_t j = tid; j < nh; j += kEsThreads) a = a + yv[j] * gv[j];
    a = es_sum<kWave>(a);
    if (lane == 0) red[wave] = a;
    __syncthreads();
    const float t = (red[0] + red[1]) + (red[2] + red[3]);
#pragma unroll kEsHubUnroll
    for (int32_t j = tid; j < nh; j += kEsThreads) o[j] = yv[j] * (gv[j] - t);
    __syncthreads();  // red is free for the tile's next hub
  }
}

// ------------------------------------------------------------------------------ entry points
// Checks shared by both directions: `ins` are the nin f32 [E] inputs.
static int es_check(const std::string& w, const int32_t* ptr, const float* const* ins, int nin,
                    const float* out, int32_t N, int64_t E) {
  MAXK_CHECK_ARG(N >= 0 && E >= 0 && E <= (int64_t)INT32_MAX, w + "sizes out of range");
  if (E == 0 || N == 0) return MAXK_OK;
  bool null = !ptr || !out;
  for (int i = 0; i < nin; ++i) null = null || !ins[i];
  MAXK_CHECK_ARG(!null, w + "null pointer");
  bool overlap = ranges_overlap(out, 4 * E, ptr, 4 * ((int64_t)N + 1));
  for (int i = 0; i < nin; ++i) overlap = overlap || ranges_overlap(out, 4 * E, ins[i], 4 * E);
  MAXK_CHECK_ARG(!overlap, w + "the output overlaps an input");
  return MAXK_OK;
}

static dim3 es_grid(int32_t N) {
  return dim3((unsigned)(((int64_t)N + kEsTileRows - 1) / kEsTileRows));
}

}  // namespace maxk

extern "C" int maxk_edge_softmax_forward(const int32_t* ptr, const float* logits, float* out,
                                         int32_t num_rows, int64_t num_edges, void* stream) {
  using namespace maxk;
  const float* ins[1] = {logits};
  const int rc = es_check("maxk_edge_softmax_forward: ", ptr, ins, 1, out, num_rows, num_edges);
  if (rc != MAXK_OK || num_edges == 0 || num_rows == 0) return rc;
  hipLaunchKernelGGL(edge_softmax_fwd_kernel, es_grid(num_rows), dim3(kEsThreads), 0,
                     (hipStream_t)stream, ptr, logits, out, num_rows, num_edges);
  MAXK_LAUNCH_CHECK("maxk_edge_softmax_forward launch");
  return MAXK_OK;
}

extern "C" int maxk_edge_softmax_backward(const int32_t* ptr, const float* y, const float* grad_y,
                                          float* grad_logits, int32_t num_rows, int64_t num_edges,
                                          void* stream) {
  using namespace maxk;
  const float* ins[2] = {y, grad_y};
  const int rc =
      es_check("maxk_edge_softmax_backward: ", ptr, ins, 2, grad_logits, num_rows, num_edges);
  if (rc != MAXK_OK || num_edges == 0 || num_rows == 0) return rc;
  hipLaunchKernelGGL(edge_softmax_bwd_kernel, es_grid(num_rows), dim3(kEsThreads), 0,
                     (hipStream_t)stream, ptr, y, grad_y, grad_logits, num_rows, num_edges);
  MAXK_LAUNCH_CHECK("maxk_edge_softmax_backward launch");
  return MAXK_OK;
}

extern "C" int maxk_edge_softmax_row_limits(int32_t* out, int32_t capacity) {
  const int32_t limits[2] = {maxk::kEsShortMax, maxk::kEsMediumMax};
  for (int i = 0; i < 2 && out && i < capacity; ++i) out[i] = limits[i];
  return 2;
}
