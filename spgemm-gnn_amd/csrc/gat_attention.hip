// GAT attention on the CSR graph (include/maxk_hip.h, "GAT attention"): the node scores el, er
// become the edge softmax in one pass, and its gradient comes back as the per-edge gradient, its
// row sums (grad_er) and, through maxk_edge_colsum, its column sums (grad_el).
//
//   forward   z = el[idx[e]] + er[r],  x = z > 0 ? z : z * slope,  alpha = edge softmax of x
//   backward  ge = alpha (g - sum_row alpha g),  grad_edge = z > 0 ? ge : ge * slope,
//             grad_er[r] = sum_row grad_edge
//   colsum    out[c] = sum_{j in column c} values[order[j]]
//
// The softmax itself is edge_softmax.h, unchanged: the forward hands it a source that gathers and
// scores instead of reading a logits array, the backward a post that applies the leaky-relu
// branch, so alpha and grad_edge carry the bits of maxk_edge_softmax_* on the materialised x by
// construction. The two sums reuse its placement (element j in lane j % W, slot j / W, slots in
// order, balanced tree, hubs (w0 + w1) + (w2 + w3)): no atomics, a row's or column's bits depend
// on its own values, their order and its length.
//
// er[r] is one value per row (per 16-lane group, wave or work-group). el[idx[j]] is a dependent
// gather: the index loads of all of a lane's slots are issued together, then the el loads, so S
// gathers are in flight per lane; el is N floats and stays in L2. A hub row of the forward gathers
// once: its first pass parks the scores in the row's place of alpha and the other two read them
// back (es_fwd_hub<true>); gathering again on every pass measured 0.995 ms against 0.745 ms on
// the Reddit-shaped graph and 1.50 against 1.42 ms on the ogbn-products-shaped one.
// The column sum reads values through order, a 4-byte gather into an [E] array.
#include "edge_softmax.h"

#include <cmath>

// every product, difference and sum below is one IEEE operation: with contraction on, z * slope
// and the subtraction of the row maximum would fuse
#pragma clang fp contract(off)

namespace maxk {

__device__ __forceinline__ int32_t gat_clamp(int32_t c, int32_t hi) {
  return c < 0 ? 0 : (c > hi ? hi : c);
}

// Element j of a row's scores: idx at the row's segment, el [num_cols], er_r the row's own score.
// idx is clamped into [0, num_cols) before use, as es_segment clamps ptr.
struct GatScore {
  const int32_t* __restrict__ idx;
  const float* __restrict__ el;
  float er_r, slope;
  int32_t col_hi;
  __device__ __forceinline__ float z(int32_t j) const {
    return el[gat_clamp(idx[j], col_hi)] + er_r;
  }
  __device__ __forceinline__ float operator()(int32_t j) const {
    const float v = z(j);
    return v > 0.f ? v : v * slope;
  }
  // as a post of the softmax backward: the score beside the gradient, then its branch
  __device__ __forceinline__ float load(int32_t j) const { return z(j); }
  __device__ __forceinline__ float apply(float zj, float ge) const {
    return zj > 0.f ? ge : ge * slope;
  }
};

// Element j of a column: values [E] through order at the column's segment, clamped into [0, E).
struct GatPermuted {
  const int32_t* __restrict__ order;
  const float* __restrict__ values;
  int32_t edge_hi;
  __device__ __forceinline__ float operator()(int32_t j) const {
    return values[gat_clamp(order[j], edge_hi)];
  }
};

__device__ __forceinline__ float gat_row_score(const float* __restrict__ er, int64_t row,
                                               int32_t num_rows) {
  return er[row < num_rows ? row : num_rows - 1];
}

// ---------------------------------------------------------------------------------- forward
// The tile logic of edge_softmax_fwd_kernel with GatScore for EsArray.
__global__ __launch_bounds__(kEsThreads) void gat_attention_fwd_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ el, const float* __restrict__ er, float slope,
    float* __restrict__ out, int32_t num_rows, int32_t num_cols, int64_t E) {
  __shared__ float red[2 * kEsWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kEsTileRows;
  const int32_t col_hi = num_cols - 1;

  int64_t b;
  int32_t n;
  const int64_t row = row0 + wave * kEsWaveRows + lane / kEsGroup;
  es_segment(ptr, row, num_rows, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  if (__ballot(ns > 0) != 0) {
    // a group with no short row scores edge 0 (E > 0) and writes nothing
    const int64_t bs = ns > 0 ? b : 0;
    const GatScore src{idx + bs, el, gat_row_score(er, row, num_rows), slope, col_hi};
    es_fwd_regs<kEsGroup, kEsShortSlots>(src, out + bs, ns, lane % kEsGroup);
  }
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    const GatScore src{idx + bg, el, er[row0 + wave * kEsWaveRows + g], slope, col_hi};
    es_fwd_medium(src, out + bg, ng, lane);
  }

  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    es_segment(ptr, row0 + r, num_rows, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    const GatScore src{idx + bh, el, er[row0 + r], slope, col_hi};
    es_fwd_hub<true>(src, out + bh, nh, tid, lane, wave, red);
  }
}

// --------------------------------------------------------------------------------- backward
// The tile logic of edge_softmax_bwd_kernel with GatScore as the post, plus the row sum of what
// was stored: every row of the grid's range writes its grad_er, an empty one +0.0f.
__global__ __launch_bounds__(kEsThreads) void gat_attention_bwd_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ el, const float* __restrict__ er, float slope,
    const float* __restrict__ y, const float* __restrict__ gy, float* __restrict__ out,
    float* __restrict__ grad_er, int32_t num_rows, int32_t num_cols, int64_t E) {
  __shared__ float red[kEsWaves];
  __shared__ float red2[kEsWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kEsTileRows;
  const int32_t col_hi = num_cols - 1;

  int64_t b;
  int32_t n;
  const int64_t row = row0 + wave * kEsWaveRows + lane / kEsGroup;
  es_segment(ptr, row, num_rows, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  float s = 0.f;
  if (__ballot(ns > 0) != 0) {
    const int64_t bs = ns > 0 ? b : 0;
    const GatScore post{idx + bs, el, gat_row_score(er, row, num_rows), slope, col_hi};
    s = es_sum<kEsGroup>(es_bwd_regs<kEsGroup, kEsShortSlots>(y + bs, gy + bs, out + bs, ns,
                                                              lane % kEsGroup, post));
  }
  if (row < num_rows && n <= kEsShortMax && lane % kEsGroup == 0) grad_er[row] = s;
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    const int64_t rg = row0 + wave * kEsWaveRows + g;
    const GatScore post{idx + bg, el, er[rg], slope, col_hi};
    const float sg = es_sum<kWave>(es_bwd_medium(y + bg, gy + bg, out + bg, ng, lane, post));
    if (lane == 0) grad_er[rg] = sg;
  }

  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    es_segment(ptr, row0 + r, num_rows, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    const GatScore post{idx + bh, el, er[row0 + r], slope, col_hi};
    const float acc = es_bwd_hub(y + bh, gy + bh, out + bh, nh, tid, lane, wave, red, post);
    const float sh = es_hub_combine(acc, lane, wave, red2);  // its barrier frees red
    if (tid == 0) grad_er[row0 + r] = sh;
    // red2 is written again only behind the next hub's first barrier
  }
}

// ------------------------------------------------------------------------------- column sum
__global__ __launch_bounds__(kEsThreads) void edge_colsum_kernel(
    const int32_t* __restrict__ ptr_t, const int32_t* __restrict__ order,
    const float* __restrict__ values, float* __restrict__ out, int32_t num_cols, int64_t E) {
  __shared__ float red[kEsWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t col0 = (int64_t)blockIdx.x * kEsTileRows;
  const int32_t edge_hi = (int32_t)(E - 1);

  int64_t b;
  int32_t n;
  const int64_t col = col0 + wave * kEsWaveRows + lane / kEsGroup;
  es_segment(ptr_t, col, num_cols, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  float s = 0.f;
  if (__ballot(ns > 0) != 0) {
    const int64_t bs = ns > 0 ? b : 0;
    s = es_sum_regs<kEsGroup, kEsShortSlots>(GatPermuted{order + bs, values, edge_hi}, ns,
                                             lane % kEsGroup);
  }
  if (col < num_cols && n <= kEsShortMax && lane % kEsGroup == 0) out[col] = s;
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    const float sg = es_sum_medium(GatPermuted{order + bg, values, edge_hi}, ng, lane);
    if (lane == 0) out[col0 + wave * kEsWaveRows + g] = sg;
  }

  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    es_segment(ptr_t, col0 + r, num_cols, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    const GatPermuted src{order + bh, values, edge_hi};
    float a = 0.f;
#pragma unroll kEsHubUnroll
    for (int32_t j = tid; j < nh; j += kEsThreads) a = a + src(j);
    const float sh = es_hub_combine(a, lane, wave, red);
    if (tid == 0) out[col0 + r] = sh;
    __syncthreads();  // red is free for the tile's next hub
  }
}

// ------------------------------------------------------------------------------ entry points
struct GatRange {
  const void* p;
  int64_t bytes;
};

// null pointers with edges, and an output that shares a byte with an input or another output
static int gat_check_ranges(const std::string& w, const GatRange* ins, int nin,
                            const GatRange* outs, int nout) {
  bool null = false;
  for (int i = 0; i < nin; ++i) null = null || (ins[i].bytes > 0 && !ins[i].p);
  for (int i = 0; i < nout; ++i) null = null || (outs[i].bytes > 0 && !outs[i].p);
  MAXK_CHECK_ARG(!null, w + "null pointer");
  bool overlap = false;
  for (int o = 0; o < nout; ++o) {
    for (int i = 0; i < nin; ++i)
      overlap = overlap || ranges_overlap(outs[o].p, outs[o].bytes, ins[i].p, ins[i].bytes);
    for (int i = o + 1; i < nout; ++i)
      overlap = overlap || ranges_overlap(outs[o].p, outs[o].bytes, outs[i].p, outs[i].bytes);
  }
  MAXK_CHECK_ARG(!overlap, w + "an output overlaps an input or another output");
  return MAXK_OK;
}

static int gat_check_sizes(const std::string& w, int32_t num_rows, int32_t num_cols, int64_t E) {
  MAXK_CHECK_ARG(num_rows >= 0 && num_cols >= 0 && E >= 0 && E <= (int64_t)INT32_MAX,
                 w + "sizes out of range");
  return MAXK_OK;
}

}  // namespace maxk

extern "C" int maxk_gat_attention_forward(const int32_t* ptr, const int32_t* idx, const float* el,
                                          const float* er, float negative_slope, float* alpha,
                                          int32_t num_rows, int32_t num_cols, int64_t num_edges,
                                          void* stream) {
  using namespace maxk;
  const std::string w = "maxk_gat_attention_forward: ";
  int rc = gat_check_sizes(w, num_rows, num_cols, num_edges);
  if (rc != MAXK_OK) return rc;
  MAXK_CHECK_ARG(std::isfinite(negative_slope), w + "negative_slope must be finite");
  if (num_edges == 0 || num_rows == 0) return MAXK_OK;
  MAXK_CHECK_ARG(num_cols > 0, w + "sizes out of range: edges without columns");
  const int64_t E = num_edges;
  const GatRange ins[4] = {{ptr, 4 * ((int64_t)num_rows + 1)}, {idx, 4 * E},
                           {el, 4 * (int64_t)num_cols}, {er, 4 * (int64_t)num_rows}};
  const GatRange outs[1] = {{alpha, 4 * E}};
  rc = gat_check_ranges(w, ins, 4, outs, 1);
  if (rc != MAXK_OK) return rc;
  hipLaunchKernelGGL(gat_attention_fwd_kernel, es_grid(num_rows), dim3(kEsThreads), 0,
                     (hipStream_t)stream, ptr, idx, el, er, negative_slope, alpha, num_rows,
                     num_cols, E);
  MAXK_LAUNCH_CHECK("maxk_gat_attention_forward launch");
  return MAXK_OK;
}

extern "C" int maxk_gat_attention_backward(const int32_t* ptr, const int32_t* idx, const float* el,
                                           const float* er, float negative_slope,
                                           const float* alpha, const float* grad_alpha,
                                           float* grad_edge, float* grad_er, int32_t num_rows,
                                           int32_t num_cols, int64_t num_edges, void* stream) {
  using namespace maxk;
  const std::string w = "maxk_gat_attention_backward: ";
  int rc = gat_check_sizes(w, num_rows, num_cols, num_edges);
  if (rc != MAXK_OK) return rc;
  MAXK_CHECK_ARG(std::isfinite(negative_slope), w + "negative_slope must be finite");
  if (num_rows == 0) return MAXK_OK;
  const int64_t E = num_edges;
  if (E == 0) {  // no edge, so every row is empty: grad_er is zeros and grad_edge has no element
    MAXK_CHECK_ARG(grad_er, w + "null pointer");
    MAXK_HIP_TRY(hipMemsetAsync(grad_er, 0, 4 * (size_t)num_rows, (hipStream_t)stream));
    return MAXK_OK;
  }
  MAXK_CHECK_ARG(num_cols > 0, w + "sizes out of range: edges without columns");
  const GatRange ins[6] = {{ptr, 4 * ((int64_t)num_rows + 1)}, {idx, 4 * E},
                           {el, 4 * (int64_t)num_cols}, {er, 4 * (int64_t)num_rows},
                           {alpha, 4 * E}, {grad_alpha, 4 * E}};
  const GatRange outs[2] = {{grad_edge, 4 * E}, {grad_er, 4 * (int64_t)num_rows}};
  rc = gat_check_ranges(w, ins, 6, outs, 2);
  if (rc != MAXK_OK) return rc;
  hipLaunchKernelGGL(gat_attention_bwd_kernel, es_grid(num_rows), dim3(kEsThreads), 0,
                     (hipStream_t)stream, ptr, idx, el, er, negative_slope, alpha, grad_alpha,
                     grad_edge, grad_er, num_rows, num_cols, E);
  MAXK_LAUNCH_CHECK("maxk_gat_attention_backward launch");
  return MAXK_OK;
}

extern "C" int maxk_edge_colsum(const int32_t* ptr_t, const int32_t* order, const float* values,
                                float* out, int32_t num_cols, int64_t num_edges, void* stream) {
  using namespace maxk;
  const std::string w = "maxk_edge_colsum: ";
  int rc = gat_check_sizes(w, 0, num_cols, num_edges);
  if (rc != MAXK_OK) return rc;
  if (num_cols == 0) return MAXK_OK;
  const int64_t E = num_edges;
  if (E == 0) {
    MAXK_CHECK_ARG(out, w + "null pointer");
    MAXK_HIP_TRY(hipMemsetAsync(out, 0, 4 * (size_t)num_cols, (hipStream_t)stream));
    return MAXK_OK;
  }
  const GatRange ins[3] = {{ptr_t, 4 * ((int64_t)num_cols + 1)}, {order, 4 * E}, {values, 4 * E}};
  const GatRange outs[1] = {{out, 4 * (int64_t)num_cols}};
  rc = gat_check_ranges(w, ins, 3, outs, 1);
  if (rc != MAXK_OK) return rc;
  hipLaunchKernelGGL(edge_colsum_kernel, es_grid(num_cols), dim3(kEsThreads), 0,
                     (hipStream_t)stream, ptr_t, order, values, out, num_cols, E);
  MAXK_LAUNCH_CHECK("maxk_edge_colsum launch");
  return MAXK_OK;
}
