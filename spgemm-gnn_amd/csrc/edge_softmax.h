// Device functions of the edge softmax (edge_softmax.hip), shared with the kernels that compute
// their logits on the fly (gat_attention.hip): the regimes by row length, the lane and slot of
// every element and the trees live here once, so a kernel that hands these functions another
// source of the same values produces the same bits by construction.
//
// A *source* is any object with `float operator()(int32_t j) const`, element j of the row it was
// made for: EsArray reads an array, the attention kernels gather and score. A *post* turns the
// softmax gradient of element j into what is stored (EsNoPost stores it as it is).
#pragma once

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
static_assert(kEsWaves == 4, "the hub rows combine four waves");

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

// Element j of a row that is an array.
struct EsArray {
  const float* __restrict__ x;
  __device__ __forceinline__ float operator()(int32_t j) const { return x[j]; }
};

// The gradient as it is; nothing to load beside it.
struct EsNoPost {
  __device__ __forceinline__ float load(int32_t) const { return 0.f; }
  __device__ __forceinline__ float apply(float, float ge) const { return ge; }
};

// ---------------------------------------------------------------------------------- forward
// W lanes (lane `sub` of them) hold S slots each of the row src(0 .. n), n in [0, W * S]. Loads
// are unconditional at a clamped index (an in-bounds element for a group with no row), so all S
// are in flight together.
template <int W, int S, class Src>
__device__ __forceinline__ void es_fwd_regs(const Src src, float* __restrict__ out, int32_t n,
                                            int sub) {
  float v[S];
  const int32_t last = n > 0 ? n - 1 : 0;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int32_t j = sub + W * i;
    v[i] = src(j < last ? j : last);
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

// A medium row (kEsShortMax < n <= kEsMediumMax) by its wave: the smallest S with 64 S >= n.
template <class Src>
__device__ __forceinline__ void es_fwd_medium(const Src src, float* __restrict__ o, int32_t n,
                                              int lane) {
  if (n <= 2 * kWave) es_fwd_regs<kWave, 2>(src, o, n, lane);
  else if (n <= 4 * kWave) es_fwd_regs<kWave, 4>(src, o, n, lane);
  else if (n <= 8 * kWave) es_fwd_regs<kWave, 8>(src, o, n, lane);
  else es_fwd_regs<kWave, kEsMediumSlots>(src, o, n, lane);
}

// A hub row by the whole work-group, the row read three times; red holds 2 * kEsWaves floats.
// Ends with a barrier: red is free for the tile's next hub. Stage: the first pass parks each
// element in its place of the output and the other two read it back from there (a thread reads
// only what it stored itself, j = tid + 256 i in every pass), for a source that costs more than a
// load; the values, and so the bits, are the same either way.
template <bool Stage = false, class Src>
__device__ __forceinline__ void es_fwd_hub(const Src src, float* __restrict__ o, int32_t nh,
                                           int tid, int lane, int wave, float* red) {
  float m = -INFINITY;
#pragma unroll kEsHubUnroll
  for (int32_t j = tid; j < nh; j += kEsThreads) {
    const float v = src(j);
    if (Stage) o[j] = v;
    m = fmaxf(m, v);
  }
  m = es_max<kWave>(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float a = 0.f;
#pragma unroll kEsHubUnroll
  for (int32_t j = tid; j < nh; j += kEsThreads) a = a + expf((Stage ? o[j] : src(j)) - m);
  a = es_sum<kWave>(a);
  if (lane == 0) red[kEsWaves + wave] = a;
  __syncthreads();
  const float inv = 1.0f / ((red[kEsWaves] + red[kEsWaves + 1]) +
                            (red[kEsWaves + 2] + red[kEsWaves + 3]));
#pragma unroll kEsHubUnroll
  for (int32_t j = tid; j < nh; j += kEsThreads) o[j] = expf((Stage ? o[j] : src(j)) - m) * inv;
  __syncthreads();
}

// --------------------------------------------------------------------------------- backward
// Stores post(y (g - t)) and returns the lane's own sum of what it stored, slots in order
// (unused, and removed, where nothing is summed).
template <int W, int S, class Post>
__device__ __forceinline__ float es_bwd_regs(const float* __restrict__ y,
                                             const float* __restrict__ gy, float* __restrict__ out,
                                             int32_t n, int sub, const Post post) {
  float v[S], g[S], q[S];
  const int32_t last = n > 0 ? n - 1 : 0;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int32_t j = sub + W * i;
    v[i] = y[j < last ? j : last];
    g[i] = gy[j < last ? j : last];
    q[i] = post.load(j < last ? j : last);
  }
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) a = a + (sub + W * i < n ? v[i] * g[i] : 0.f);
  const float t = es_sum<W>(a);
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const float o = post.apply(q[i], v[i] * (g[i] - t));
    if (sub + W * i < n) out[sub + W * i] = o;
    acc = acc + (sub + W * i < n ? o : 0.f);
  }
  return acc;
}

template <class Post>
__device__ __forceinline__ float es_bwd_medium(const float* __restrict__ y,
                                               const float* __restrict__ gy,
                                               float* __restrict__ o, int32_t n, int lane,
                                               const Post post) {
  if (n <= 2 * kWave) return es_bwd_regs<kWave, 2>(y, gy, o, n, lane, post);
  if (n <= 4 * kWave) return es_bwd_regs<kWave, 4>(y, gy, o, n, lane, post);
  if (n <= 8 * kWave) return es_bwd_regs<kWave, 8>(y, gy, o, n, lane, post);
  return es_bwd_regs<kWave, kEsMediumSlots>(y, gy, o, n, lane, post);
}

// A hub row by the whole work-group; red holds kEsWaves floats and is in use until the caller's
// next barrier. Returns the thread's own sum of what it stored.
template <class Post>
__device__ __forceinline__ float es_bwd_hub(const float* __restrict__ yv,
                                            const float* __restrict__ gv, float* __restrict__ o,
                                            int32_t nh, int tid, int lane, int wave,
                                            float* red, const Post post) {
  float a = 0.f;
#pragma unroll kEsHubUnroll
  for (int32_t j = tid; j < nh; j += kEsThreads) a = a + yv[j] * gv[j];
  a = es_sum<kWave>(a);
  if (lane == 0) red[wave] = a;
  __syncthreads();
  const float t = (red[0] + red[1]) + (red[2] + red[3]);
  float acc = 0.f;
#pragma unroll kEsHubUnroll
  for (int32_t j = tid; j < nh; j += kEsThreads) {
    const float ov = post.apply(post.load(j), yv[j] * (gv[j] - t));
    o[j] = ov;
    acc = acc + ov;
  }
  return acc;
}

// -------------------------------------------------------------------------------------- sum
// The sum of the row src(0 .. n) alone, in the placement of the two functions above: element j
// in lane j % W, slot j / W, a lane's slots in order, then the butterfly.
template <int W, int S, class Src>
__device__ __forceinline__ float es_sum_regs(const Src src, int32_t n, int sub) {
  float v[S];
  const int32_t last = n > 0 ? n - 1 : 0;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int32_t j = sub + W * i;
    v[i] = src(j < last ? j : last);
  }
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) a = a + (sub + W * i < n ? v[i] : 0.f);
  return es_sum<W>(a);
}

template <class Src>
__device__ __forceinline__ float es_sum_medium(const Src src, int32_t n, int lane) {
  if (n <= 2 * kWave) return es_sum_regs<kWave, 2>(src, n, lane);
  if (n <= 4 * kWave) return es_sum_regs<kWave, 4>(src, n, lane);
  if (n <= 8 * kWave) return es_sum_regs<kWave, 8>(src, n, lane);
  return es_sum_regs<kWave, kEsMediumSlots>(src, n, lane);
}

// Combines the four waves' sums of a hub row as (w0 + w1) + (w2 + w3); every thread gets the
// result. red holds kEsWaves floats and is in use until the caller's next barrier.
__device__ __forceinline__ float es_hub_combine(float a, int lane, int wave, float* red) {
  a = es_sum<kWave>(a);
  if (lane == 0) red[wave] = a;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

static inline dim3 es_grid(int32_t N) {
  return dim3((unsigned)(((int64_t)N + kEsTileRows - 1) / kEsTileRows));
}

}  // namespace maxk
