// Multi-head aggregation on MaxK features (include/maxk_hip.h, "Multi-head aggregation"): every
// CBSR slot of a source column is weighed by the attention of its own head, hd(s) = s / F.
//
//   forward    out[r, s]       = sum_{e in row r}        alpha[hd(s), e] * X[idx[e], s]
//   backward   grad_sp[c, l]   = sum_{j in column c}     alpha[hd(s), e] * grad_out[r, s]
//              grad_alpha[h,e] = sum_{l: hd(s) = h}      sp_data[c, l]   * grad_out[r, s]
//              with e = order[j], r = idx_t[j], s = sp_index[c, l]
//
// No plan, no scratch, no global atomics: both kernels read the plain [num_cols, k] tables and the
// CSR (forward) or the transposed structure (backward) as they are. Lane groups, the tile and its
// three passes, and the backward's combination of the groups' sums are lane_groups.h. Edges of a
// group are taken in order, the groups' partial sums are combined by a balanced tree in a fixed
// order, so a row's bits depend on its own inputs and its length alone.
//
// Forward: a group accumulates its edges into its own D-wide LDS row with ds_add_f32 (a column's
// slots are distinct features, so the lanes of an edge do not collide; a repeated selector
// collides and the LDS serialises the two adds). Rows of different groups are combined when the
// row is written. Backward: a lane keeps grad_sp of its slot in a register across the column's
// out-edges; the products sp_data * grad_out of an edge are reduced per head by a reduce-scatter
// butterfly over HP head places (HP - 1 shuffles, then log2(LP / HP) more), which leaves head
// bitrev(sub) in lane sub < HP: no sort of the slots, no LDS, every (h, e) stored once.
#include "common.h"
#include "variants_heads.h"

namespace maxk_mh {

using maxk::check_ranges;
using maxk::clampi;
using maxk::kWave;
using maxk::Range;
using maxk::set_error;
using maxk::lg::wave_lds_sync;

__device__ __forceinline__ void lds_add(float* p, float v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // ds_add_f32
}

// p[0] + p[stride] + ... over N = 2^m places as a balanced tree
template <int N>
__device__ __forceinline__ float tree(const float* p, int stride) {
  if constexpr (N == 1) {
    return p[0];
  } else {
    return tree<N / 2>(p, stride) + tree<N / 2>(p + (N / 2) * stride, stride);
  }
}

// ---------------------------------------------------------------------------------- forward
struct FwdArgs {
  const int32_t* ptr;
  const int32_t* idx;
  const float* alpha;
  const float* data;
  int64_t ds;
  const uint8_t* sel;
  int64_t is;
  float* out;
  int32_t num_rows, num_cols;
  int64_t E;
  int32_t D, k;
  uint32_t magic;
};

constexpr int kFwdEdgesInFlight = 4;

// Edges first, first + step, ... of the row at [b, b + n) into acc (D floats of LDS).
template <int LP>
__device__ __forceinline__ void fwd_edges(const FwdArgs& a, float* acc, int64_t b, int32_t n,
                                          int first, int step, int sub) {
  constexpr int U = kFwdEdgesInFlight;
  const int32_t col_hi = a.num_cols - 1;
  const uint32_t sel_hi = (uint32_t)(a.D - 1);
  for (int64_t j0 = first; j0 < n; j0 += (int64_t)step * U) {
    int64_t c[U], e[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * step;
      ok[u] = j < n;
      e[u] = b + (ok[u] ? j : (int64_t)n - 1);  // an edge of the row either way
      c[u] = clampi(a.idx[e[u]], col_hi);
    }
    for (int l = sub; l < a.k; l += LP) {
      uint32_t s[U];
      float v[U], w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t raw = a.sel[c[u] * a.is + l];
        s[u] = raw < sel_hi ? raw : sel_hi;
        v[u] = a.data[c[u] * a.ds + l];
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        w[u] = a.alpha[(int64_t)heads_head_of((int)s[u], a.magic) * a.E + e[u]];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[u]) lds_add(acc + s[u], w[u] * v[u]);
    }
  }
}

template <int LP>
__global__ __launch_bounds__(lg::kThreads) void heads_fwd_kernel(const FwdArgs a) {
  extern __shared__ float lds[];  // NG accumulator rows of D + 1 floats
  const lg::Place<LP> p{};
  constexpr int G = p.G, NG = p.NG;
  const int D = a.D, stride = a.D + 1;
  float* mine = lds + p.gid * stride;
  float* wacc = lds + p.wave * G * stride;
  const int64_t row0 = (int64_t)blockIdx.x * lg::kTile;

  // its edges in order
  lg::short_rows(p, a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
    for (int j = p.sub; j < D; j += LP) mine[j] = 0.f;
    wave_lds_sync();
    fwd_edges<LP>(a, mine, b, n, 0, 1, p.sub);
    wave_lds_sync();
    for (int j = p.sub; j < D; j += LP) a.out[row * D + j] = mine[j];
    wave_lds_sync();
  });

  lg::medium_rows(p, a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
    for (int j = p.lane; j < G * stride; j += kWave) wacc[j] = 0.f;
    wave_lds_sync();
    fwd_edges<LP>(a, mine, b, n, p.g, G, p.sub);
    wave_lds_sync();
    for (int j = p.lane; j < D; j += kWave) a.out[row * D + j] = tree<G>(wacc + j, stride);
    wave_lds_sync();
  });

  lg::hub_rows(a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
    __syncthreads();  // every wave is done with its accumulators
    for (int j = p.tid; j < NG * stride; j += lg::kThreads) lds[j] = 0.f;
    __syncthreads();
    fwd_edges<LP>(a, mine, b, n, p.gid, NG, p.sub);
    __syncthreads();
    for (int j = p.tid; j < D; j += lg::kThreads) a.out[row * D + j] = tree<NG>(lds + j, stride);
  });
}

// --------------------------------------------------------------------------------- backward
struct BwdArgs {
  const int32_t* ptr_t;
  const int32_t* idx_t;
  const int32_t* order;
  const float* alpha;
  const float* grad_out;
  int64_t gs;
  const float* data;
  int64_t ds;
  const uint8_t* sel;
  int64_t is;
  float* grad_sp;     // may be null
  float* grad_alpha;  // may be null
  int32_t H, num_rows, num_cols;
  int64_t E;
  int32_t D, k;
  uint32_t magic;
};

constexpr int kBwdEdgesInFlight = 2;

// The head that lane `sub` < HP holds after the reduce-scatter: bit t of sub chose the upper half
// at stage t, i.e. head bit log2(HP) - 1 - t.
template <int HP>
__device__ __forceinline__ int held_head(int sub) {
  int h = 0;
#pragma unroll
  for (int t = 0; (1 << t) < HP; ++t) h |= ((sub >> t) & 1) * (HP >> (t + 1));
  return h;
}

// Transposed entries first, first + step, ... of column c at [b, b + n): adds into gsp[i] the
// lane's slots' terms (when grad_sp is wanted) and stores grad_alpha of each entry's edge.
template <int LP, int HP, int S>
__device__ __forceinline__ void bwd_edges(const BwdArgs& a, int64_t c, int64_t b, int32_t n,
                                          int first, int step, int sub, float (&gsp)[S]) {
  constexpr int U = kBwdEdgesInFlight;
  const bool want_sp = a.grad_sp != nullptr, want_alpha = a.grad_alpha != nullptr;
  const uint32_t sel_hi = (uint32_t)(a.D - 1);
  uint32_t s[S];
  int h[S];
  float x[S];
  bool on[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int l = sub + LP * i;
    on[i] = l < a.k;
    const uint32_t raw = on[i] ? a.sel[c * a.is + l] : 0u;
    s[i] = raw < sel_hi ? raw : sel_hi;
    h[i] = heads_head_of((int)s[i], a.magic);
    x[i] = on[i] && want_alpha ? a.data[c * a.ds + l] : 0.f;  // no sp_data read without grad_alpha
  }
  const int mine = held_head<HP>(sub);
  const bool writer = sub < HP && mine < a.H;
  const int32_t edge_hi = (int32_t)(a.E - 1), row_hi = a.num_rows - 1;

  for (int64_t j0 = first; j0 < n; j0 += (int64_t)step * U) {
    int64_t e[U], r[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * step;
      ok[u] = j < n;
      const int64_t jj = b + (ok[u] ? j : (int64_t)n - 1);
      e[u] = clampi(a.order[jj], edge_hi);
      r[u] = clampi(a.idx_t[jj], row_hi);
    }
    float gv[U][S];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < S; ++i) gv[u][i] = on[i] ? a.grad_out[r[u] * a.gs + s[i]] : 0.f;
    if (want_sp) {
      float w[U][S];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < S; ++i) w[u][i] = on[i] ? a.alpha[(int64_t)h[i] * a.E + e[u]] : 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < S; ++i)
          if (ok[u] && on[i]) gsp[i] = gsp[i] + w[u][i] * gv[u][i];
    }
    if (want_alpha) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float v[HP];
#pragma unroll
        for (int q = 0; q < HP; ++q) v[q] = 0.f;
#pragma unroll
        for (int i = 0; i < S; ++i) {
          const float p = x[i] * gv[u][i];
#pragma unroll
          for (int q = 0; q < HP; ++q)
            if (on[i] && h[i] == q) v[q] = v[q] + p;
        }
        // reduce-scatter over the HP lanes that share sub / HP: each stage halves the heads a
        // lane holds and adds the partner's terms of the half it keeps
#pragma unroll
        for (int t = 0; (1 << t) < HP; ++t) {
          const int half = HP >> (t + 1);
          const bool up = (sub >> t) & 1;
#pragma unroll
          for (int q = 0; q < half; ++q) {
            const float send = up ? v[q] : v[q + half];
            const float keep = up ? v[q + half] : v[q];
            v[q] = keep + __shfl_xor(send, 1 << t, kWave);
          }
        }
        float tot = v[0];
#pragma unroll
        for (int m = HP; m < LP; m <<= 1) tot = tot + __shfl_xor(tot, m, kWave);
        if (writer && ok[u]) a.grad_alpha[(int64_t)mine * a.E + e[u]] = tot;
      }
    }
  }
}

template <int LP, int HP>
__global__ __launch_bounds__(lg::kThreads) void heads_bwd_kernel(const BwdArgs a) {
  static_assert(LP >= HP, "the reduce-scatter ends with one head per lane");
  constexpr int S = lg::lane_slots(LP);
  __shared__ float red[lg::kWaves][maxk::kMaxDim];
  const lg::Place<LP> p{};
  const int k = a.k;
  const int64_t col0 = (int64_t)blockIdx.x * lg::kTile;

  // grad_sp may be null: then the passes are there for grad_alpha, which bwd_edges stores
  lg::short_rows(p, a.ptr_t, col0, a.num_cols, a.E, [&](int64_t col, int64_t b, int32_t n) {
    float gsp[S] = {};
    bwd_edges<LP, HP, S>(a, col, b, n, 0, 1, p.sub, gsp);
    if (a.grad_sp) lg::store_group(p, gsp, k, a.grad_sp, col);
  });

  lg::medium_rows(p, a.ptr_t, col0, a.num_cols, a.E, [&](int64_t col, int64_t b, int32_t n) {
    float gsp[S] = {};
    bwd_edges<LP, HP, S>(a, col, b, n, p.g, p.G, p.sub, gsp);
    if (a.grad_sp) lg::reduce_wave_and_store(p, gsp, k, a.grad_sp, col);
  });

  lg::hub_rows(a.ptr_t, col0, a.num_cols, a.E, [&](int64_t col, int64_t b, int32_t n) {
    float gsp[S] = {};
    bwd_edges<LP, HP, S>(a, col, b, n, p.gid, p.NG, p.sub, gsp);
    if (a.grad_sp) lg::reduce_block_and_store(p, gsp, k, a.grad_sp, col, red);
  });
}

// ------------------------------------------------------------------------------ entry points
// sizes, k, heads and strides shared by both calls; strides are resolved (0: the row width)
static int check_shape(const std::string& w, int32_t H, int32_t num_rows, int32_t num_cols,
                       int64_t E, int32_t D, int32_t k, int64_t& ds, int64_t& is) {
  return lg::check_shape(w, num_rows, num_cols, E, D, k, is, [&]() -> int {
    MAXK_CHECK_ARG(H >= 1 && D % H == 0, w + "num_heads must be >= 1 and divide dim_origin");
    if ((D / H) % 4 != 0) {
      set_error(w + "dim_origin / num_heads must be a multiple of 4");
      return MAXK_ERR_UNSUPPORTED;
    }
    if (H > kHeadsMaxHeads) {
      set_error(w + "num_heads above 16 is not supported");
      return MAXK_ERR_UNSUPPORTED;
    }
    if (ds == 0) ds = k;
    MAXK_CHECK_ARG(ds >= k, w + "data_stride must be >= k (0: k)");
    return MAXK_OK;
  });
}

static int forward_impl(const int32_t* ptr, const int32_t* idx, const float* alpha,
                        const float* sp_data, int64_t ds, const uint8_t* sp_index, int64_t is,
                        float* out, int32_t H, int32_t N, int32_t NC, int64_t E, int32_t D,
                        int32_t k, void* stream) {
  const std::string w("maxk_heads_aggregate_forward: ");
  int rc = check_shape(w, H, N, NC, E, D, k, ds, is);
  if (rc != MAXK_OK) return rc;
  if (N == 0) return MAXK_OK;
  MAXK_CHECK_ARG(out, w + "null pointer");
  if (E == 0) {  // every row is empty
    MAXK_HIP_TRY(hipMemsetAsync(out, 0, 4 * (size_t)N * (size_t)D, (hipStream_t)stream));
    return MAXK_OK;
  }
  const Range ins[5] = {{ptr, 4 * ((int64_t)N + 1)},
                        {idx, 4 * E},
                        {alpha, 4 * H * E},
                        {sp_data, 4 * ((int64_t)(NC - 1) * ds + k)},
                        {sp_index, (int64_t)(NC - 1) * is + k}};
  const Range outs[1] = {{out, 4 * (int64_t)N * D}};
  rc = check_ranges(w, ins, 5, outs, 1);
  if (rc != MAXK_OK) return rc;
  const FwdArgs a{ptr, idx, alpha, sp_data, ds, sp_index, is, out, N, NC, E, D, k,
                  heads_magic(D / H)};
  if (int e = maxk::dispatch_variant(
          kHeadsFwdVariants, select_heads_fwd_variant(k), [&](auto i) -> int {
            constexpr int LP = kHeadsFwdVariants[decltype(i)::value].lp;
            const size_t lds = sizeof(float) * (size_t)(lg::kThreads / LP) * (size_t)(D + 1);
            hipLaunchKernelGGL(heads_fwd_kernel<LP>, lg::tile_grid(N), dim3(lg::kThreads), lds,
                               (hipStream_t)stream, a);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_heads_aggregate_forward launch");
  return MAXK_OK;
}

static int backward_impl(const int32_t* ptr_t, const int32_t* idx_t, const int32_t* order,
                         const float* alpha, const float* grad_out, int64_t gs,
                         const float* sp_data, int64_t ds, const uint8_t* sp_index, int64_t is,
                         float* grad_sp, float* grad_alpha, int32_t H, int32_t N, int32_t NC,
                         int64_t E, int32_t D, int32_t k, void* stream) {
  const std::string w("maxk_heads_aggregate_backward: ");
  int rc = check_shape(w, H, N, NC, E, D, k, ds, is);
  if (rc != MAXK_OK) return rc;
  if (gs == 0) gs = D;
  MAXK_CHECK_ARG(gs >= D, w + "grad_stride must be >= dim_origin (0: dim_origin)");
  if (!grad_sp && !grad_alpha) return MAXK_OK;  // nothing asked for: no gather
  if (NC == 0) return MAXK_OK;
  if (E == 0) {  // every column is empty; grad_alpha has no element
    if (grad_sp)
      MAXK_HIP_TRY(hipMemsetAsync(grad_sp, 0, 4 * (size_t)NC * (size_t)k, (hipStream_t)stream));
    return MAXK_OK;
  }
  // alpha is read for grad_sp only, sp_data for grad_alpha only
  const Range ins[7] = {{ptr_t, 4 * ((int64_t)NC + 1)},
                        {idx_t, 4 * E},
                        {order, 4 * E},
                        {alpha, grad_sp ? 4 * H * E : 0},
                        {grad_out, 4 * ((int64_t)(N - 1) * gs + D)},
                        {sp_data, grad_alpha ? 4 * ((int64_t)(NC - 1) * ds + k) : 0},
                        {sp_index, (int64_t)(NC - 1) * is + k}};
  const Range outs[2] = {{grad_sp, grad_sp ? 4 * (int64_t)NC * k : 0},
                         {grad_alpha, grad_alpha ? 4 * H * E : 0}};
  rc = check_ranges(w, ins, 7, outs, 2);
  if (rc != MAXK_OK) return rc;
  const BwdArgs a{ptr_t, idx_t, order, alpha, grad_out, gs, sp_data, ds, sp_index, is, grad_sp,
                  grad_alpha, H, N, NC, E, D, k, heads_magic(D / H)};
  if (int e = maxk::dispatch_variant(
          kHeadsBwdVariants, select_heads_bwd_variant(k, H), [&](auto i) -> int {
            constexpr HeadsBwdVariant v = kHeadsBwdVariants[decltype(i)::value];
            hipLaunchKernelGGL((heads_bwd_kernel<v.lp, v.hp>), lg::tile_grid(NC),
                               dim3(lg::kThreads), 0, (hipStream_t)stream, a);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_heads_aggregate_backward launch");
  return MAXK_OK;
}

}  // namespace maxk_mh

extern "C" int maxk_heads_aggregate_forward(const int32_t* ptr, const int32_t* idx,
                                            const float* alpha, const float* sp_data,
                                            int64_t data_stride, const uint8_t* sp_index,
                                            int64_t index_stride, float* out, int32_t num_heads,
                                            int32_t num_rows, int32_t num_cols, int64_t num_edges,
                                            int32_t dim_origin, int32_t dim_k, void* stream) {
  return maxk_mh::forward_impl(ptr, idx, alpha, sp_data, data_stride, sp_index, index_stride, out,
                               num_heads, num_rows, num_cols, num_edges, dim_origin, dim_k,
                               stream);
}

extern "C" int maxk_heads_aggregate_backward(
    const int32_t* ptr_t, const int32_t* idx_t, const int32_t* order, const float* alpha,
    const float* grad_out, int64_t grad_stride, const float* sp_data, int64_t data_stride,
    const uint8_t* sp_index, int64_t index_stride, float* grad_sp, float* grad_alpha,
    int32_t num_heads, int32_t num_rows, int32_t num_cols, int64_t num_edges, int32_t dim_origin,
    int32_t dim_k, void* stream) {
  return maxk_mh::backward_impl(ptr_t, idx_t, order, alpha, grad_out, grad_stride, sp_data,
                                data_stride, sp_index, index_stride, grad_sp, grad_alpha,
                                num_heads, num_rows, num_cols, num_edges, dim_origin, dim_k,
                                stream);
}

extern "C" int maxk_heads_row_limits(int32_t* out, int32_t capacity) {
  namespace lg = maxk::lg;
  return maxk::copy_limits(out, capacity,
                           {lg::kShortMax, lg::kMediumMax, lg::kShortMax, lg::kMediumMax});
}
