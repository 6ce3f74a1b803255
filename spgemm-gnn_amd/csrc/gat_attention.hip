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

// Element j of a row's scores: idx at the row's segment, el [num_cols], er_r the row's own score.
// idx is clamped into [0, num_cols) before use, as row_segment clamps ptr.
struct GatScore {
  const int32_t* __restrict__ idx;
  const float* __restrict__ el;
  float er_r, slope;
  int32_t col_hi;
  __device__ __forceinline__ float z(int32_t j) const {
    return el[clampi(idx[j], col_hi)] + er_r;
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
    return values[clampi(order[j], edge_hi)];
  }
};

__device__ __forceinline__ float gat_row_score(const float* __restrict__ er, int64_t row,
                                               int32_t num_rows) {
  return er[row < num_rows ? row : num_rows - 1];
}

// The kernels' bodies are the three .inc files beside this one, included by the single-head
// kernel and by its head-batched twin: the single-head kernels compile from exactly the statements
// they always had (an inlined device function gave other register allocation and branch polarity).
// ---------------------------------------------------------------------------------- forward
// The tile logic of edge_softmax_fwd_kernel with GatScore for EsArray.
__global__ __launch_bounds__(kEsThreads) void gat_attention_fwd_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ el, const float* __restrict__ er, float slope,
    float* __restrict__ out, int32_t num_rows, int32_t num_cols, int64_t E) {
#include "gat_attention_fwd.inc"
}

// --------------------------------------------------------------------------------- backward
// The tile logic of edge_softmax_bwd_kernel with GatScore as the post, plus the row sum of what
// was stored: every row of the grid's range writes its grad_er, an empty one +0.0f.
__global__ __launch_bounds__(kEsThreads) void gat_attention_bwd_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ el, const float* __restrict__ er, float slope,
    const float* __restrict__ y, const float* __restrict__ gy, float* __restrict__ out,
    float* __restrict__ grad_er, int32_t num_rows, int32_t num_cols, int64_t E) {
#include "gat_attention_bwd.inc"
}

// ------------------------------------------------------------------------------- column sum
__global__ __launch_bounds__(kEsThreads) void edge_colsum_kernel(
    const int32_t* __restrict__ ptr_t, const int32_t* __restrict__ order,
    const float* __restrict__ values, float* __restrict__ out, int32_t num_cols, int64_t E) {
#include "edge_colsum.inc"
}

}  // namespace maxk

// The head-batched kernels (include/maxk_hip.h, "GAT attention, heads"): the same bodies on head
// blockIdx.y of the head-major arrays, so head h of a batched call carries the bits of the
// single-head call on row h by construction. Kernels of their own, outside namespace maxk
// (DESIGN section 4.12).
namespace maxk_mh {

using namespace maxk;

__global__ __launch_bounds__(kEsThreads) void gat_attention_fwd_heads_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ el, const float* __restrict__ er, float slope,
    float* __restrict__ out, int32_t num_rows, int32_t num_cols, int64_t E) {
  el += (int64_t)blockIdx.y * num_cols;
  er += (int64_t)blockIdx.y * num_rows;
  out += (int64_t)blockIdx.y * E;
#include "gat_attention_fwd.inc"
}

__global__ __launch_bounds__(kEsThreads) void gat_attention_bwd_heads_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ el, const float* __restrict__ er, float slope,
    const float* __restrict__ y, const float* __restrict__ gy, float* __restrict__ out,
    float* __restrict__ grad_er, int32_t num_rows, int32_t num_cols, int64_t E) {
  el += (int64_t)blockIdx.y * num_cols;
  er += (int64_t)blockIdx.y * num_rows;
  y += (int64_t)blockIdx.y * E;
  gy += (int64_t)blockIdx.y * E;
  out += (int64_t)blockIdx.y * E;
  grad_er += (int64_t)blockIdx.y * num_rows;
#include "gat_attention_bwd.inc"
}

__global__ __launch_bounds__(kEsThreads) void edge_colsum_heads_kernel(
    const int32_t* __restrict__ ptr_t, const int32_t* __restrict__ order,
    const float* __restrict__ values, float* __restrict__ out, int32_t num_cols, int64_t E) {
  values += (int64_t)blockIdx.y * E;
  out += (int64_t)blockIdx.y * num_cols;
#include "edge_colsum.inc"
}

}  // namespace maxk_mh

namespace maxk {

// ------------------------------------------------------------------------------ entry points
static int gat_check_sizes(const std::string& w, int32_t num_rows, int32_t num_cols, int64_t E) {
  MAXK_CHECK_ARG(num_rows >= 0 && num_cols >= 0 && E >= 0 && E <= (int64_t)INT32_MAX,
                 w + "sizes out of range");
  return MAXK_OK;
}

// The head-major arrays of H heads: H within the grid's second dimension, and every array's
// byte size (4 H times its per-head length) within int64.
static int gat_check_heads(const std::string& w, int32_t H, int32_t num_rows, int32_t num_cols,
                           int64_t E) {
  MAXK_CHECK_ARG(H >= 1, w + "num_heads must be >= 1");
  int64_t longest = E > num_rows ? E : num_rows;
  longest = longest > num_cols ? longest : num_cols;
  MAXK_CHECK_ARG(H <= 65535 && (int64_t)H <= (INT64_MAX / 4) / (longest > 0 ? longest : 1),
                 w + "num_heads * num_edges is beyond what the offsets can address");
  return MAXK_OK;
}

static dim3 gat_grid(int32_t n, int32_t H) {
  dim3 g = es_grid(n);
  g.y = (unsigned)H;
  return g;
}

static int gat_forward_impl(const std::string& w, const int32_t* ptr, const int32_t* idx,
                            const float* el, const float* er, float negative_slope, float* alpha,
                            bool heads, int32_t H, int32_t num_rows, int32_t num_cols,
                            int64_t num_edges, void* stream) {
  int rc = gat_check_sizes(w, num_rows, num_cols, num_edges);
  if (rc != MAXK_OK) return rc;
  rc = gat_check_heads(w, H, num_rows, num_cols, num_edges);
  if (rc != MAXK_OK) return rc;
  MAXK_CHECK_ARG(std::isfinite(negative_slope), w + "negative_slope must be finite");
  if (num_edges == 0 || num_rows == 0) return MAXK_OK;
  MAXK_CHECK_ARG(num_cols > 0, w + "sizes out of range: edges without columns");
  const int64_t E = num_edges;
  const Range ins[4] = {{ptr, 4 * ((int64_t)num_rows + 1)}, {idx, 4 * E},
                           {el, 4 * H * (int64_t)num_cols}, {er, 4 * H * (int64_t)num_rows}};
  const Range outs[1] = {{alpha, 4 * H * E}};
  rc = check_ranges(w, ins, 4, outs, 1);
  if (rc != MAXK_OK) return rc;
  if (heads)
    hipLaunchKernelGGL(maxk_mh::gat_attention_fwd_heads_kernel, gat_grid(num_rows, H),
                       dim3(kEsThreads), 0, (hipStream_t)stream, ptr, idx, el, er, negative_slope,
                       alpha, num_rows, num_cols, E);
  else
    hipLaunchKernelGGL(gat_attention_fwd_kernel, es_grid(num_rows), dim3(kEsThreads), 0,
                       (hipStream_t)stream, ptr, idx, el, er, negative_slope, alpha, num_rows,
                       num_cols, E);
  MAXK_LAUNCH_CHECK((w + "launch").c_str());
  return MAXK_OK;
}

static int gat_backward_impl(const std::string& w, const int32_t* ptr, const int32_t* idx,
                             const float* el, const float* er, float negative_slope,
                             const float* alpha, const float* grad_alpha, float* grad_edge,
                             float* grad_er, bool heads, int32_t H, int32_t num_rows,
                             int32_t num_cols, int64_t num_edges, void* stream) {
  int rc = gat_check_sizes(w, num_rows, num_cols, num_edges);
  if (rc != MAXK_OK) return rc;
  rc = gat_check_heads(w, H, num_rows, num_cols, num_edges);
  if (rc != MAXK_OK) return rc;
  MAXK_CHECK_ARG(std::isfinite(negative_slope), w + "negative_slope must be finite");
  if (num_rows == 0) return MAXK_OK;
  const int64_t E = num_edges;
  if (E == 0) {  // no edge, so every row is empty: grad_er is zeros and grad_edge has no element
    MAXK_CHECK_ARG(grad_er, w + "null pointer");
    MAXK_HIP_TRY(hipMemsetAsync(grad_er, 0, 4 * (size_t)H * (size_t)num_rows,
                                (hipStream_t)stream));
    return MAXK_OK;
  }
  MAXK_CHECK_ARG(num_cols > 0, w + "sizes out of range: edges without columns");
  const Range ins[6] = {{ptr, 4 * ((int64_t)num_rows + 1)}, {idx, 4 * E},
                           {el, 4 * H * (int64_t)num_cols}, {er, 4 * H * (int64_t)num_rows},
                           {alpha, 4 * H * E}, {grad_alpha, 4 * H * E}};
  const Range outs[2] = {{grad_edge, 4 * H * E}, {grad_er, 4 * H * (int64_t)num_rows}};
  rc = check_ranges(w, ins, 6, outs, 2);
  if (rc != MAXK_OK) return rc;
  if (heads)
    hipLaunchKernelGGL(maxk_mh::gat_attention_bwd_heads_kernel, gat_grid(num_rows, H),
                       dim3(kEsThreads), 0, (hipStream_t)stream, ptr, idx, el, er, negative_slope,
                       alpha, grad_alpha, grad_edge, grad_er, num_rows, num_cols, E);
  else
    hipLaunchKernelGGL(gat_attention_bwd_kernel, es_grid(num_rows), dim3(kEsThreads), 0,
                       (hipStream_t)stream, ptr, idx, el, er, negative_slope, alpha, grad_alpha,
                       grad_edge, grad_er, num_rows, num_cols, E);
  MAXK_LAUNCH_CHECK((w + "launch").c_str());
  return MAXK_OK;
}

static int gat_colsum_impl(const std::string& w, const int32_t* ptr_t, const int32_t* order,
                           const float* values, float* out, bool heads, int32_t H,
                           int32_t num_cols, int64_t num_edges, void* stream) {
  int rc = gat_check_sizes(w, 0, num_cols, num_edges);
  if (rc != MAXK_OK) return rc;
  rc = gat_check_heads(w, H, 0, num_cols, num_edges);
  if (rc != MAXK_OK) return rc;
  if (num_cols == 0) return MAXK_OK;
  const int64_t E = num_edges;
  if (E == 0) {
    MAXK_CHECK_ARG(out, w + "null pointer");
    MAXK_HIP_TRY(hipMemsetAsync(out, 0, 4 * (size_t)H * (size_t)num_cols, (hipStream_t)stream));
    return MAXK_OK;
  }
  const Range ins[3] = {{ptr_t, 4 * ((int64_t)num_cols + 1)}, {order, 4 * E},
                           {values, 4 * H * E}};
  const Range outs[1] = {{out, 4 * H * (int64_t)num_cols}};
  rc = check_ranges(w, ins, 3, outs, 1);
  if (rc != MAXK_OK) return rc;
  if (heads)
    hipLaunchKernelGGL(maxk_mh::edge_colsum_heads_kernel, gat_grid(num_cols, H), dim3(kEsThreads),
                       0, (hipStream_t)stream, ptr_t, order, values, out, num_cols, E);
  else
    hipLaunchKernelGGL(edge_colsum_kernel, es_grid(num_cols), dim3(kEsThreads), 0,
                       (hipStream_t)stream, ptr_t, order, values, out, num_cols, E);
  MAXK_LAUNCH_CHECK((w + "launch").c_str());
  return MAXK_OK;
}

}  // namespace maxk

extern "C" int maxk_gat_attention_forward(const int32_t* ptr, const int32_t* idx, const float* el,
                                          const float* er, float negative_slope, float* alpha,
                                          int32_t num_rows, int32_t num_cols, int64_t num_edges,
                                          void* stream) {
  return maxk::gat_forward_impl("maxk_gat_attention_forward: ", ptr, idx, el, er, negative_slope,
                                alpha, false, 1, num_rows, num_cols, num_edges, stream);
}

extern "C" int maxk_gat_attention_forward_heads(const int32_t* ptr, const int32_t* idx,
                                                const float* el, const float* er,
                                                float negative_slope, float* alpha,
                                                int32_t num_heads, int32_t num_rows,
                                                int32_t num_cols, int64_t num_edges,
                                                void* stream) {
  return maxk::gat_forward_impl("maxk_gat_attention_forward_heads: ", ptr, idx, el, er,
                                negative_slope, alpha, true, num_heads, num_rows, num_cols,
                                num_edges, stream);
}

extern "C" int maxk_gat_attention_backward(const int32_t* ptr, const int32_t* idx, const float* el,
                                           const float* er, float negative_slope,
                                           const float* alpha, const float* grad_alpha,
                                           float* grad_edge, float* grad_er, int32_t num_rows,
                                           int32_t num_cols, int64_t num_edges, void* stream) {
  return maxk::gat_backward_impl("maxk_gat_attention_backward: ", ptr, idx, el, er,
                                 negative_slope, alpha, grad_alpha, grad_edge, grad_er, false, 1,
                                 num_rows, num_cols, num_edges, stream);
}

extern "C" int maxk_gat_attention_backward_heads(const int32_t* ptr, const int32_t* idx,
                                                 const float* el, const float* er,
                                                 float negative_slope, const float* alpha,
                                                 const float* grad_alpha, float* grad_edge,
                                                 float* grad_er, int32_t num_heads,
                                                 int32_t num_rows, int32_t num_cols,
                                                 int64_t num_edges, void* stream) {
  return maxk::gat_backward_impl("maxk_gat_attention_backward_heads: ", ptr, idx, el, er,
                                 negative_slope, alpha, grad_alpha, grad_edge, grad_er, true,
                                 num_heads, num_rows, num_cols, num_edges, stream);
}

extern "C" int maxk_edge_colsum(const int32_t* ptr_t, const int32_t* order, const float* values,
                                float* out, int32_t num_cols, int64_t num_edges, void* stream) {
  return maxk::gat_colsum_impl("maxk_edge_colsum: ", ptr_t, order, values, out, false, 1,
                               num_cols, num_edges, stream);
}

extern "C" int maxk_edge_colsum_heads(const int32_t* ptr_t, const int32_t* order,
                                      const float* values, float* out, int32_t num_heads,
                                      int32_t num_cols, int64_t num_edges, void* stream) {
  return maxk::gat_colsum_impl("maxk_edge_colsum_heads: ", ptr_t, order, values, out, true,
                               num_heads, num_cols, num_edges, stream);
}
