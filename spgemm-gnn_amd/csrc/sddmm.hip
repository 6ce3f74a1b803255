// Sampled dense-dense product per edge: the gradient of the SpGEMM forward with respect to
// the edge values (include/maxk_hip.h, "Edge-value gradient").
//
//   grad_val[e] = sum_{l<k} sp_data[c, l] * grad_out[r, sp_index[c, l]]      e = (r, c)
//
// summed in the balanced pairwise tree over adjacent slots that the header pins.
//
// Shape: one 256-thread work-group per fixed chunk of kSddmmChunk CSR edges, no plan. The
// chunk's first and last destination rows come from two wave-uniform binary searches of ptr;
// every thread then finds the rows of its four edges by a search between those two (no step
// for a hub row that spans the chunk, empty rows never visited) and leaves {row, column} of
// each edge in LDS. An edge is served by LP = K2 / 4 adjacent lanes (K2 the next power of two
// >= k, one lane for K2 < 4), each holding four adjacent slots: at k % 4 == 0 one 16-B load
// of four values and one 4-B word of four selectors per lane, scalar loads per slot
// otherwise. The sampled grad_out elements are read through the vector cache: one row is
// shared by all of a row's edges. Staging the chunk's rows in LDS measured slower, and four
// edges in flight per lane group no faster. A lane sums its four
// products pairwise, then log2(LP) xor butterflies finish the tree.
#include "common.h"

// every product and every sum below is one IEEE operation: no fused multiply-add
#pragma clang fp contract(off)

namespace maxk {

constexpr int kSddmmThreads = 256;
constexpr int kSddmmChunk = 1024;  // CSR edges per work-group

// First r in [lo, hi) with ptr[r] > e (hi if none): row(e) = that - 1.
__device__ __forceinline__ int32_t first_row_past(const int32_t* __restrict__ ptr, int32_t lo,
                                                  int32_t hi, int64_t e) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)ptr[mid] > e) hi = mid; else lo = mid + 1;
  }
  return lo;
}

template <int LP>
__global__ __launch_bounds__(kSddmmThreads) void sddmm_edge_grad_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
    const float* __restrict__ grad_out, int64_t gs, const float* __restrict__ sp_data, int64_t ds,
    const uint8_t* __restrict__ sp_index, int64_t is, float* __restrict__ grad_val,
    int32_t num_rows, int64_t E, int32_t k, int32_t K2) {
  __shared__ int32_t rowof[kSddmmChunk];  // the chunk's edges: destination row, source column
  __shared__ int32_t colof[kSddmmChunk];

  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * kSddmmChunk;
  const int32_t n = (int32_t)((E - e0 < kSddmmChunk) ? E - e0 : kSddmmChunk);
  // wave-uniform: rows of the chunk's first and last edge (clamped: a ptr that breaks the
  // documented preconditions still indexes inside the arrays)
  int32_t rlo = first_row_past(ptr, 0, num_rows, e0) - 1;
  int32_t rhi = first_row_past(ptr, 0, num_rows, e0 + n - 1) - 1;
  rlo = rlo < 0 ? 0 : rlo;
  rhi = rhi < rlo ? rlo : rhi;
  for (int i = tid; i < n; i += kSddmmThreads) {
    rowof[i] = first_row_past(ptr, rlo + 1, rhi + 1, e0 + i) - 1;
    colof[i] = idx[e0 + i];
  }
  __syncthreads();

  constexpr int G = kSddmmThreads / LP;  // edges per work-group step
  const int gid = tid / LP, sub = tid % LP;
  const int l0 = sub * 4;
  const bool vec = (k & 3) == 0;
  for (int i = gid; i < n; i += G) {  // the lanes of a group share i
    const int64_t c = colof[i];
    const float* xv = sp_data + c * ds;
    const uint8_t* xs = sp_index + c * is;
    const float* g = grad_out + (int64_t)rowof[i] * gs;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t s[4] = {0, 0, 0, 0};
    if (vec) {
      if (l0 < k) {
        const float4 v = *reinterpret_cast<const float4*>(xv + l0);
        const uint32_t w = *reinterpret_cast<const uint32_t*>(xs + l0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        s[0] = w & 255u; s[1] = (w >> 8) & 255u; s[2] = (w >> 16) & 255u; s[3] = w >> 24;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (l0 + j < k) { x[j] = xv[l0 + j]; s[j] = xs[l0 + j]; }
    }
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)  // a slot past k is +0.0f, never a product (0 * Inf)
      t[j] = l0 + j < k ? x[j] * g[s[j]] : 0.f;
    float a = t[0];
    if (K2 >= 2) a = a + t[1];
    if (K2 >= 4) a = a + (t[2] + t[3]);
#pragma unroll
    for (int m = 1; m < LP; m <<= 1) a = a + __shfl_xor(a, m, kWave);
    if (sub == 0) grad_val[e0 + i] = a;
  }
}

static int sddmm_impl(const int32_t* ptr, const int32_t* idx, const float* grad_out,
                      int64_t gs, const float* sp_data, int64_t ds, const uint8_t* sp_index,
                      int64_t is, float* grad_val, int32_t N, int32_t NC, int64_t E, int32_t D,
                      int32_t k, void* stream) {
  const std::string w("maxk_sddmm_edge_grad: ");
  MAXK_CHECK_ARG(N >= 0 && NC >= 0 && E >= 0 && E <= (int64_t)INT32_MAX * kSddmmChunk,
                 w + "sizes out of range");
  MAXK_CHECK_ARG(D >= 1 && D <= kMaxDim, w + "dim_origin must be in [1, 256]");
  MAXK_CHECK_ARG(k >= 1 && k <= D, w + "k must be between 1 and input dimension");
  if (D % 4 != 0) {
    set_error(w + "dim_origin must be a multiple of 4");
    return MAXK_ERR_UNSUPPORTED;
  }
  if (gs == 0) gs = D;
  if (ds == 0) ds = k;
  if (is == 0) is = k;
  MAXK_CHECK_ARG(gs >= D, w + "grad_stride must be >= dim_origin (0: dim_origin)");
  MAXK_CHECK_ARG(ds >= k, w + "data_stride must be >= k (0: k)");
  MAXK_CHECK_ARG(is >= k, w + "index_stride must be >= k (0: k)");
  if (E == 0 || N == 0) return MAXK_OK;
  MAXK_CHECK_ARG(ptr && idx && grad_out && sp_data && sp_index && grad_val, w + "null pointer");
  MAXK_CHECK_ARG(!ranges_overlap(grad_val, 4 * E, ptr, 4 * ((int64_t)N + 1)) &&
                     !ranges_overlap(grad_val, 4 * E, idx, 4 * E) &&
                     !ranges_overlap(grad_val, 4 * E, grad_out, 4 * ((int64_t)(N - 1) * gs + D)) &&
                     !ranges_overlap(grad_val, 4 * E, sp_data, 4 * ((int64_t)(NC - 1) * ds + k)) &&
                     !ranges_overlap(grad_val, 4 * E, sp_index, (int64_t)(NC - 1) * is + k),
                 w + "grad_val overlaps an input");
  MAXK_CHECK_ARG(NC > 0, w + "num_cols must be > 0 with edges");
  const int K2 = sddmm_slots(k);
  const dim3 grid((unsigned)((E + kSddmmChunk - 1) / kSddmmChunk));
  if (int e = dispatch_variant(kSddmmVariants, select_sddmm_variant(k), [&](auto i) -> int {
        hipLaunchKernelGGL(sddmm_edge_grad_kernel<kSddmmVariants[decltype(i)::value].lanes>, grid,
                           dim3(kSddmmThreads), 0, (hipStream_t)stream, ptr, idx, grad_out, gs,
                           sp_data, ds, sp_index, is, grad_val, N, E, k, K2);
        return MAXK_OK;
      }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_sddmm_edge_grad launch");
  return MAXK_OK;
}

}  // namespace maxk

extern "C" int maxk_sddmm_edge_grad(const int32_t* ptr, const int32_t* idx,
                                    const float* grad_out, int64_t grad_stride,
                                    const float* sp_data, int64_t data_stride,
                                    const uint8_t* sp_index, int64_t index_stride,
                                    float* grad_val, int32_t num_rows, int32_t num_cols,
                                    int64_t num_edges, int32_t dim_origin, int32_t dim_k,
                                    void* stream) {
  return maxk::sddmm_impl(ptr, idx, grad_out, grad_stride, sp_data, data_stride, sp_index,
                          index_stride, grad_val, num_rows, num_cols, num_edges, dim_origin, dim_k,
                          stream);
}
