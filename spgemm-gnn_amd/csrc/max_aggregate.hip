// Max aggregation of MaxK features (include/maxk_hip.h, "Max aggregation"): the element-wise
// maximum of a row's in-neighbours, with the unselected features of a column as implicit zeros.
//
//   forward    out[r, s]     = max over the row's edges e of X[idx[e], s], with the winner's
//                              CSR edge and slot in arg_edge / arg_slot (-1, 0: the implicit zero)
//   backward   grad_sp[c, l] = sum_{j in column c} [arg_edge[r, s] == e and arg_slot[r, s] == l]
//                              * grad_out[r, s]      with e = order[j], r = idx_t[j],
//                                                    s = sp_index[c, l]
//
// No plan, no scratch, no global atomics. Lane groups, the tile and its three passes, and the
// backward's combination of the groups' sums are lane_groups.h, shared with heads_aggregate.hip.
//
// Forward: a row's state in LDS is, per feature, a 64-bit cell
//     order_key(value) << 32 | ~(j * 256 + l)          j: the edge's place in its row, l: the slot
// raised with ds_max_u64, and a 32-bit count of the edges whose column selects the feature. The
// larger key wins, equal keys go to the lowest j, then the lowest l: a total order on distinct
// candidates, so the cell's final value does not depend on the order of the updates, colliding
// lanes included. An edge counts once for a feature however many of its slots select it: the
// lanes of an edge mark the feature in a 256-bit map of their lane group (ds_or_rtn_b32) and only
// the first to mark it counts. The implicit zero competes where the count stays below the row's
// length. Backward: a lane keeps grad_sp of its slot in a register across the column's entries
// and reads grad_out only where arg_edge / arg_slot name its (edge, slot).
#include "common.h"
#include "variants_max.h"

namespace maxk_mx {

using maxk::check_ranges;
using maxk::clampi;
using maxk::kWave;
using maxk::Range;
using maxk::set_error;
using maxk::lg::wave_lds_sync;

// The order of the exact top-k (maxk_topk.hip, order_key): larger float, larger key; +0 above
// -0; every NaN is the largest key. No key is 0.
__device__ __forceinline__ uint32_t order_key(float x) {
  const uint32_t b = __float_as_uint(x);
  const uint32_t key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (b & 0x7fffffffu) > 0x7f800000u ? 0xffffffffu : key;
}
constexpr uint32_t kKeyZero = 0x80000000u;  // order_key(+0.0f)
constexpr uint32_t kKeyNaN = 0xffffffffu;

__device__ __forceinline__ void lds_max(uint64_t* p, uint64_t v) {
  __hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // ds_max_u64
}
__device__ __forceinline__ void lds_inc(uint32_t* p) {
  __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // ds_add_u32
}
__device__ __forceinline__ uint32_t lds_or(uint32_t* p, uint32_t v) {
  return __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---------------------------------------------------------------------------------- forward
struct FwdArgs {
  const int32_t* ptr;
  const int32_t* idx;
  const float* data;
  int64_t ds;
  const uint8_t* sel;
  int64_t is;
  float* out;
  int32_t* arg_edge;
  uint8_t* arg_slot;
  int32_t num_rows, num_cols;
  int64_t E;
  int32_t D, k;
};

constexpr int kFwdEdgesInFlight = 4;
constexpr int kSeenWords = maxk::kMaxDim / 32;  // a 256-bit feature map

// Edges first, first + step, ... of the row at [b, b + n) into the row's cells and counts.
// `seen`: the lane group's kFwdEdgesInFlight feature maps.
template <int LP>
__device__ __forceinline__ void fwd_edges(const FwdArgs& a, uint64_t* cell, uint32_t* hit,
                                          uint32_t* seen, int64_t b, int32_t n, int first,
                                          int step, int sub) {
  constexpr int U = kFwdEdgesInFlight;
  const int32_t col_hi = a.num_cols - 1;
  const uint32_t sel_hi = (uint32_t)(a.D - 1);
  for (int64_t j0 = first; j0 < n; j0 += (int64_t)step * U) {
    for (int w = sub; w < U * kSeenWords; w += LP) seen[w] = 0u;
    wave_lds_sync();
    int64_t c[U];
    uint32_t jw[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * step;
      ok[u] = j < n;
      const int64_t jj = ok[u] ? j : (int64_t)n - 1;  // an edge of the row either way
      c[u] = clampi(a.idx[b + jj], col_hi);
      jw[u] = (uint32_t)jj << 8;
    }
    for (int l = sub; l < a.k; l += LP) {
      uint32_t s[U];
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t raw = a.sel[c[u] * a.is + l];
        s[u] = raw < sel_hi ? raw : sel_hi;
        v[u] = a.data[c[u] * a.ds + l];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!ok[u]) continue;
        const uint32_t bit = 1u << (s[u] & 31u);
        if (!(lds_or(seen + u * kSeenWords + (s[u] >> 5), bit) & bit)) lds_inc(hit + s[u]);
        lds_max(cell + s[u], ((uint64_t)order_key(v[u]) << 32) | (uint32_t) ~(jw[u] + (uint32_t)l));
      }
    }
    wave_lds_sync();
  }
}

// Element (row, s) from its final cell and count.
template <bool ARG>
__device__ __forceinline__ void fwd_emit(const FwdArgs& a, int64_t row, int s, uint64_t cell,
                                         uint32_t hits, int64_t b, int32_t n) {
  const uint32_t key = (uint32_t)(cell >> 32);
  float v = 0.f;
  int32_t edge = -1;
  uint32_t slot = 0;
  // no candidate at all, or the implicit zero competes and ranks above the best explicit one
  if (key != 0u && !(hits < (uint32_t)n && key < kKeyZero)) {
    const uint32_t pos = ~(uint32_t)cell;
    const int64_t e = b + (int64_t)(pos >> 8);
    slot = pos & 255u;
    edge = (int32_t)e;
    if (key == kKeyNaN) {  // the key does not hold a NaN's bits
      const int64_t c = clampi(a.idx[e], a.num_cols - 1);
      v = a.data[c * a.ds + slot];
    } else {
      v = __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
    }
  }
  const int64_t o = row * a.D + s;
  a.out[o] = v;
  if constexpr (ARG) {
    a.arg_edge[o] = edge;
    a.arg_slot[o] = (uint8_t)slot;
  }
}

template <int LP, bool ARG>
__global__ __launch_bounds__(lg::kThreads) void max_fwd_kernel(const FwdArgs a) {
  extern __shared__ uint64_t lds[];  // R x D cells, R x D counts, NG x U feature maps
  const lg::Place<LP> p{};
  constexpr int G = p.G, NG = p.NG;
  constexpr int R = max_fwd_states(LP);
  static_assert(R >= lg::kWaves, "a wave has a row state of its own");
  const int D = a.D;
  uint64_t* cells = lds;
  uint32_t* hits = reinterpret_cast<uint32_t*>(cells + R * D);
  uint32_t* seen = hits + R * D + p.gid * (kFwdEdgesInFlight * kSeenWords);
  const int64_t row0 = (int64_t)blockIdx.x * lg::kTile;

  // with the row state of the group
  lg::short_rows(p, a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
    uint64_t* cell = cells + (p.gid % R) * D;
    uint32_t* hit = hits + (p.gid % R) * D;
    if (n == 0) {
      for (int j = p.sub; j < D; j += LP) fwd_emit<ARG>(a, row, j, 0u, 0u, b, n);
      return;
    }
    for (int j = p.sub; j < D; j += LP) {
      cell[j] = 0u;
      hit[j] = 0u;
    }
    wave_lds_sync();
    fwd_edges<LP>(a, cell, hit, seen, b, n, 0, 1, p.sub);
    for (int j = p.sub; j < D; j += LP) fwd_emit<ARG>(a, row, j, cell[j], hit[j], b, n);
    wave_lds_sync();
  });
  __syncthreads();  // the row states change hands: group gid's to wave `wave`

  // a wave's groups on one row state
  {
    uint64_t* cell = cells + p.wave * D;
    uint32_t* hit = hits + p.wave * D;
    lg::medium_rows(p, a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
      for (int j = p.lane; j < D; j += kWave) {
        cell[j] = 0u;
        hit[j] = 0u;
      }
      wave_lds_sync();
      fwd_edges<LP>(a, cell, hit, seen, b, n, p.g, G, p.sub);
      wave_lds_sync();
      for (int j = p.lane; j < D; j += kWave) fwd_emit<ARG>(a, row, j, cell[j], hit[j], b, n);
      wave_lds_sync();
    });
  }

  // on row state 0
  lg::hub_rows(a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
    __syncthreads();  // every wave is done with its row state
    for (int j = p.tid; j < D; j += lg::kThreads) {
      cells[j] = 0u;
      hits[j] = 0u;
    }
    __syncthreads();
    fwd_edges<LP>(a, cells, hits, seen, b, n, p.gid, NG, p.sub);
    __syncthreads();
    for (int j = p.tid; j < D; j += lg::kThreads)
      fwd_emit<ARG>(a, row, j, cells[j], hits[j], b, n);
  });
}

// --------------------------------------------------------------------------------- backward
struct BwdArgs {
  const int32_t* ptr_t;
  const int32_t* idx_t;
  const int32_t* order;
  const float* grad_out;
  int64_t gs;
  const int32_t* arg_edge;
  const uint8_t* arg_slot;
  const uint8_t* sel;
  int64_t is;
  float* grad_sp;
  int32_t num_rows, num_cols;
  int64_t E;
  int32_t D, k;
};

constexpr int kBwdEdgesInFlight = 2;

// Transposed entries first, first + step, ... of column c at [b, b + n): adds into gsp[i] the
// grad_out elements whose winner is the lane's slot i of the entry's edge.
template <int LP, int S>
__device__ __forceinline__ void bwd_edges(const BwdArgs& a, int64_t c, int64_t b, int32_t n,
                                          int first, int step, int sub, float (&gsp)[S]) {
  constexpr int U = kBwdEdgesInFlight;
  const uint32_t sel_hi = (uint32_t)(a.D - 1);
  uint32_t s[S];
  bool on[S];
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const int l = sub + LP * i;
    on[i] = l < a.k;
    const uint32_t raw = on[i] ? a.sel[c * a.is + l] : 0u;
    s[i] = raw < sel_hi ? raw : sel_hi;
  }
  const int32_t edge_hi = (int32_t)(a.E - 1), row_hi = a.num_rows - 1;

  for (int64_t j0 = first; j0 < n; j0 += (int64_t)step * U) {
    int32_t e[U];
    int64_t r[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * step;
      ok[u] = j < n;
      const int64_t jj = b + (ok[u] ? j : (int64_t)n - 1);
      e[u] = clampi(a.order[jj], edge_hi);
      r[u] = clampi(a.idx_t[jj], row_hi);
    }
    // the edge names the winner but for a repeated selector: arg_slot and grad_out are read
    // only where arg_edge matches (about one entry in a row's length)
    bool hit[U][S];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < S; ++i)
        hit[u][i] = (a.arg_edge[r[u] * a.D + s[i]] == e[u]) && ok[u] && on[i];  // a valid address
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < S; ++i)
        if (hit[u][i] && (int)a.arg_slot[r[u] * a.D + s[i]] == sub + LP * i)
          gsp[i] = gsp[i] + a.grad_out[r[u] * a.gs + s[i]];
  }
}

// The three passes and the combination of the groups' sums are written out here, not taken from
// lane_groups.h: through those helpers the compiler orders this kernel's gathers differently, and
// it measured 1 to 2 % slower in two passes out of two, which is at the edge of what the timing
// resolves (profiles/lane_groups.md). As written it compiles to the code it always had. A change to short_rows / medium_rows / hub_rows or to the epilogue functions of
// lane_groups.h has to be made here too.
template <int LP>
__global__ __launch_bounds__(lg::kThreads) void max_bwd_kernel(const BwdArgs a) {
  constexpr int S = lg::lane_slots(LP);
  __shared__ float red[lg::kWaves][maxk::kMaxDim];
  const lg::Place<LP> p{};
  const int k = a.k;
  const int64_t col0 = (int64_t)blockIdx.x * lg::kTile;
  int64_t b;
  int32_t n;
  float gsp[S];

  // short columns (and empty ones): one lane group each
  for (int t = p.gid; t < lg::kTile; t += p.NG) {
    const int64_t col = col0 + t;
    maxk::row_segment(a.ptr_t, col, a.num_cols, a.E, b, n);
    if (col >= a.num_cols || n > lg::kShortMax) continue;
#pragma unroll
    for (int i = 0; i < S; ++i) gsp[i] = 0.f;
    bwd_edges<LP, S>(a, col, b, n, 0, 1, p.sub, gsp);
#pragma unroll
    for (int i = 0; i < S; ++i)
      if (p.sub + LP * i < k) a.grad_sp[col * k + p.sub + LP * i] = gsp[i];
  }

  // medium columns: one wave each (wave-uniform branch), groups combined by a butterfly
  for (int t = p.wave; t < lg::kTile; t += lg::kWaves) {
    const int64_t col = col0 + t;
    maxk::row_segment(a.ptr_t, col, a.num_cols, a.E, b, n);
    if (n <= lg::kShortMax || n > lg::kMediumMax) continue;
#pragma unroll
    for (int i = 0; i < S; ++i) gsp[i] = 0.f;
    bwd_edges<LP, S>(a, col, b, n, p.g, p.G, p.sub, gsp);
#pragma unroll
    for (int i = 0; i < S; ++i) {
#pragma unroll
      for (int m = LP; m < kWave; m <<= 1) gsp[i] = gsp[i] + __shfl_xor(gsp[i], m, kWave);
      if (p.g == 0 && p.sub + LP * i < k) a.grad_sp[col * k + p.sub + LP * i] = gsp[i];
    }
  }

  // hub columns: the whole work-group (block-uniform branch), waves as (w0 + w1) + (w2 + w3)
  for (int t = 0; t < lg::kTile; ++t) {
    const int64_t col = col0 + t;
    maxk::row_segment(a.ptr_t, col, a.num_cols, a.E, b, n);
    if (n <= lg::kMediumMax) continue;
#pragma unroll
    for (int i = 0; i < S; ++i) gsp[i] = 0.f;
    bwd_edges<LP, S>(a, col, b, n, p.gid, p.NG, p.sub, gsp);
    __syncthreads();  // red is free (the tile's previous hub was read)
#pragma unroll
    for (int i = 0; i < S; ++i) {
#pragma unroll
      for (int m = LP; m < kWave; m <<= 1) gsp[i] = gsp[i] + __shfl_xor(gsp[i], m, kWave);
      if (p.g == 0 && p.sub + LP * i < k) red[p.wave][p.sub + LP * i] = gsp[i];
    }
    __syncthreads();
    for (int l = p.tid; l < k; l += lg::kThreads)
      a.grad_sp[col * k + l] = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
  }
}

// ------------------------------------------------------------------------------ entry points
static int forward_impl(const int32_t* ptr, const int32_t* idx, const float* sp_data, int64_t ds,
                        const uint8_t* sp_index, int64_t is, float* out, int32_t* arg_edge,
                        uint8_t* arg_slot, int32_t N, int32_t NC, int64_t E, int32_t D, int32_t k,
                        void* stream) {
  const std::string w("maxk_max_aggregate_forward: ");
  int rc = lg::check_shape(w, N, NC, E, D, k, is);
  if (rc != MAXK_OK) return rc;
  if (ds == 0) ds = k;
  MAXK_CHECK_ARG(ds >= k, w + "data_stride must be >= k (0: k)");
  MAXK_CHECK_ARG((arg_edge == nullptr) == (arg_slot == nullptr),
                 w + "arg_edge and arg_slot must both be given or both be NULL");
  if (N == 0) return MAXK_OK;
  MAXK_CHECK_ARG(out, w + "null pointer");
  const bool arg = arg_edge != nullptr;
  const int64_t cells = (int64_t)N * D;
  const Range outs[3] = {{out, 4 * cells}, {arg_edge, arg ? 4 * cells : 0},
                         {arg_slot, arg ? cells : 0}};
  if (E == 0) {  // every row is empty: (+0.0f, -1, 0)
    rc = check_ranges(w, nullptr, 0, outs, 3);
    if (rc != MAXK_OK) return rc;
    MAXK_HIP_TRY(hipMemsetAsync(out, 0, 4 * (size_t)cells, (hipStream_t)stream));
    if (arg) {
      MAXK_HIP_TRY(hipMemsetAsync(arg_edge, 0xff, 4 * (size_t)cells, (hipStream_t)stream));
      MAXK_HIP_TRY(hipMemsetAsync(arg_slot, 0, (size_t)cells, (hipStream_t)stream));
    }
    return MAXK_OK;
  }
  const Range ins[4] = {{ptr, 4 * ((int64_t)N + 1)},
                        {idx, 4 * E},
                        {sp_data, 4 * ((int64_t)(NC - 1) * ds + k)},
                        {sp_index, (int64_t)(NC - 1) * is + k}};
  rc = check_ranges(w, ins, 4, outs, 3);
  if (rc != MAXK_OK) return rc;
  const FwdArgs a{ptr, idx, sp_data, ds, sp_index, is, out, arg_edge, arg_slot, N, NC, E, D, k};
  if (int e = maxk::dispatch_variant(
          kMaxFwdVariants, select_max_fwd_variant(k, arg), [&](auto i) -> int {
            constexpr MaxFwdVariant v = kMaxFwdVariants[decltype(i)::value];
            const size_t lds = (size_t)max_fwd_states(v.lp) * (size_t)D * 12 +
                               (size_t)(lg::kThreads / v.lp) * kFwdEdgesInFlight * kSeenWords * 4;
            hipLaunchKernelGGL((max_fwd_kernel<v.lp, v.arg>), lg::tile_grid(N),
                               dim3(lg::kThreads), lds, (hipStream_t)stream, a);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_max_aggregate_forward launch");
  return MAXK_OK;
}

static int backward_impl(const int32_t* ptr_t, const int32_t* idx_t, const int32_t* order,
                         const float* grad_out, int64_t gs, const int32_t* arg_edge,
                         const uint8_t* arg_slot, const uint8_t* sp_index, int64_t is,
                         float* grad_sp, int32_t N, int32_t NC, int64_t E, int32_t D, int32_t k,
                         void* stream) {
  const std::string w("maxk_max_aggregate_backward: ");
  int rc = lg::check_shape(w, N, NC, E, D, k, is);
  if (rc != MAXK_OK) return rc;
  if (gs == 0) gs = D;
  MAXK_CHECK_ARG(gs >= D, w + "grad_stride must be >= dim_origin (0: dim_origin)");
  if (NC == 0) return MAXK_OK;
  MAXK_CHECK_ARG(grad_sp, w + "null pointer");
  if (E == 0) {  // every column is empty
    MAXK_HIP_TRY(hipMemsetAsync(grad_sp, 0, 4 * (size_t)NC * (size_t)k, (hipStream_t)stream));
    return MAXK_OK;
  }
  const Range ins[7] = {{ptr_t, 4 * ((int64_t)NC + 1)},
                        {idx_t, 4 * E},
                        {order, 4 * E},
                        {grad_out, 4 * ((int64_t)(N - 1) * gs + D)},
                        {arg_edge, 4 * (int64_t)N * D},
                        {arg_slot, (int64_t)N * D},
                        {sp_index, (int64_t)(NC - 1) * is + k}};
  const Range outs[1] = {{grad_sp, 4 * (int64_t)NC * k}};
  rc = check_ranges(w, ins, 7, outs, 1);
  if (rc != MAXK_OK) return rc;
  const BwdArgs a{ptr_t, idx_t, order, grad_out, gs, arg_edge, arg_slot, sp_index, is, grad_sp,
                  N, NC, E, D, k};
  if (int e = maxk::dispatch_variant(
          kMaxBwdVariants, select_max_bwd_variant(k), [&](auto i) -> int {
            constexpr int LP = kMaxBwdVariants[decltype(i)::value].lp;
            hipLaunchKernelGGL(max_bwd_kernel<LP>, lg::tile_grid(NC), dim3(lg::kThreads), 0,
                               (hipStream_t)stream, a);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_max_aggregate_backward launch");
  return MAXK_OK;
}

}  // namespace maxk_mx

extern "C" int maxk_max_aggregate_forward(const int32_t* ptr, const int32_t* idx,
                                          const float* sp_data, int64_t data_stride,
                                          const uint8_t* sp_index, int64_t index_stride,
                                          float* out, int32_t* arg_edge, uint8_t* arg_slot,
                                          int32_t num_rows, int32_t num_cols, int64_t num_edges,
                                          int32_t dim_origin, int32_t dim_k, void* stream) {
  return maxk_mx::forward_impl(ptr, idx, sp_data, data_stride, sp_index, index_stride, out,
                               arg_edge, arg_slot, num_rows, num_cols, num_edges, dim_origin,
                               dim_k, stream);
}

extern "C" int maxk_max_aggregate_backward(const int32_t* ptr_t, const int32_t* idx_t,
                                           const int32_t* order, const float* grad_out,
                                           int64_t grad_stride, const int32_t* arg_edge,
                                           const uint8_t* arg_slot, const uint8_t* sp_index,
                                           int64_t index_stride, float* grad_sp, int32_t num_rows,
                                           int32_t num_cols, int64_t num_edges,
                                           int32_t dim_origin, int32_t dim_k, void* stream) {
  return maxk_mx::backward_impl(ptr_t, idx_t, order, grad_out, grad_stride, arg_edge, arg_slot,
                                sp_index, index_stride, grad_sp, num_rows, num_cols, num_edges,
                                dim_origin, dim_k, stream);
}

extern "C" int maxk_max_row_limits(int32_t* out, int32_t capacity) {
  namespace lg = maxk::lg;
  return maxk::copy_limits(out, capacity,
                           {lg::kShortMax, lg::kMediumMax, lg::kShortMax, lg::kMediumMax});
}
