// Products of a CBSR matrix with a small dense table (include/maxk_hip.h, "MaxK linear layers").
// With the tables v [N, k] f32 and s [N, k] u8 of N rows that keep k of D features, and a table
// T [D, M]:
//
//   (A) matmul          out[n, :] = sum_l v[n, l] T[s[n, l], :]  (+ bias)
//   (B) sampled matmul  out[n, l] = <g[n, :], T[s[n, l], :]>
//   (C) weight grad     dT[j, :]  = sum_{(n, l): s[n, l] = j} v[n, l] g[n, :]
//                       dsum[j]   = sum_{(n, l): s[n, l] = j} v[n, l]
//
// which are N k M multiply-adds each where the dense products on the densified rows are N D M.
// No plan, no global atomics, nothing allocated.
//
// No matrix instructions: an MFMA tile multiplies dense fragments, so it would need the densified
// rows, D / k times the flops (16 x at D = 256, k = 16: 30.5 GFLOP instead of 1.9 at N = 232,965,
// M = 256), and the kernels below are bound by their one [N, M] stream well before the 1.9.
//
// Work split, common to the three: a work-group of 16 waves owns one panel of MP columns of M
// (blockIdx.y) and holds T[:, panel] in LDS, D * MP floats staged once with 16-byte loads; it then
// walks the rows blockIdx.x * 16 + wave, + gridDim.x * 16, ... one row per wave. All panels
// together are at most kLinGroups work-groups, so the panel is staged once per work-group and not
// once per block of rows. Lane i of the wave loads slot i of the row (value and selector, 64 slots
// a round), and the slot loop reads them back with v_readlane, wave-uniform; a lane owns the
// MP / 64 adjacent columns lane * MP / 64 ... of the panel, so every LDS access of a slot is one
// run of adjacent words, free of bank conflicts.
//
// (A) k LDS reads and k fused multiply-adds per lane in slot order, the bias last, one coalesced
// store. (B) the lane keeps its columns of g[n, :] in registers and forms per slot the partial
// dot product over them; kLinSlotTile = 16 partials are reduced across the wave by the
// reduce-scatter of heads_bwd_kernel (15 shuffles leave sum bitrev(lane % 16) over 16 lanes in
// every lane, 2 more finish it), so a sum is stored once, by one lane. With more than one panel
// the sums go to scratch [P][N, k] and a second kernel adds them in panel order. (C) the LDS holds
// the accumulator of dT[:, panel] instead, zeroed by the kernel; per slot the lane adds
// v[n, l] * g[n, its columns] into row s[n, l] with ds_add_f32, and lane l adds v[n, l] into the
// [D] sums (first panel only). The work-group leaves both in scratch and a second kernel adds the
// work-groups' partials in ascending order into dT and dsum, writing every element. The order of
// the LDS adds among the waves is not fixed: (C) keeps an error bound, not a summation order.
#include "common.h"
#include "variants_linear.h"

namespace maxk_lin {

using maxk::check_ranges;
using maxk::Range;
using maxk::set_error;

template <class K>
static hipError_t allow_lds(K* kernel, size_t bytes) {
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)bytes);
}

__device__ __forceinline__ void lds_add(float* p, float v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // ds_add_f32
}

constexpr int kSlotsInFlight = 4;  // of the matmul's slot loop

// Lane j's x, for a wave-uniform j
__device__ __forceinline__ float lane_value(float x, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}
__device__ __forceinline__ int lane_value(int x, int j) {
  return __builtin_amdgcn_readlane(x, j);
}

__device__ __forceinline__ int wave_of_thread() {
  return __builtin_amdgcn_readfirstlane((int)threadIdx.x / kLinWave);
}

// T[:, p0 .. p0 + MP) into lds [D][MP], columns at or past M as zeros: 16-byte loads where the
// table's base and row stride allow them and the four columns exist.
template <int MP>
__device__ __forceinline__ void stage_panel(float* lds, const float* __restrict__ T, int64_t ts,
                                            int D, int M, int p0) {
  constexpr int Q = MP / 4;
  const bool vec = (reinterpret_cast<uintptr_t>(T) & 15) == 0 && (ts & 3) == 0;
  for (int i = threadIdx.x; i < D * Q; i += kLinThreads) {
    const int j = i / Q, col = p0 + 4 * (i % Q);
    const float* src = T + (int64_t)j * ts + col;
    float4 x;
    if (vec && col + 3 < M) {
      x = *reinterpret_cast<const float4*>(src);
    } else {
      x.x = col < M ? src[0] : 0.f;
      x.y = col + 1 < M ? src[1] : 0.f;
      x.z = col + 2 < M ? src[2] : 0.f;
      x.w = col + 3 < M ? src[3] : 0.f;
    }
    reinterpret_cast<float4*>(lds)[i] = x;
  }
}

// Slots l0 + lane of row `row`: the value (0 past k) and the selector clamped into [0, D)
struct SlotRound {
  float v;
  int s;
  __device__ __forceinline__ void load(const float* __restrict__ data, int64_t ds,
                                       const uint8_t* __restrict__ sel, int64_t is, int64_t row,
                                       int l0, int lane, int k, int D) {
    const int l = l0 + lane;
    const bool on = l < k;
    v = (on && data) ? data[row * ds + l] : 0.f;
    const int raw = on ? (int)sel[row * is + l] : 0;
    s = raw < D ? raw : D - 1;
  }
};

// ------------------------------------------------------------------------------- (A) matmul
struct MatmulArgs {
  const float* data;
  int64_t ds;
  const uint8_t* sel;
  int64_t is;
  const float* T;
  int64_t ts;
  const float* bias;
  float* out;
  int64_t os;
  int32_t N, D, k, M;
};

template <int MP>
__global__ __launch_bounds__(kLinThreads) void cbsr_matmul_kernel(const MatmulArgs a) {
  extern __shared__ float lds[];  // T[:, panel], [D][MP]
  constexpr int C = MP / kLinWave;
  const int lane = threadIdx.x & (kLinWave - 1), wave = wave_of_thread();
  const int p0 = blockIdx.y * MP, col0 = p0 + lane * C;
  stage_panel<MP>(lds, a.T, a.ts, a.D, a.M, p0);
  __syncthreads();

  float b[C];
#pragma unroll
  for (int c = 0; c < C; ++c) b[c] = (a.bias && col0 + c < a.M) ? a.bias[col0 + c] : 0.f;
  const float* mine = lds + lane * C;

  for (int64_t row = (int64_t)blockIdx.x * kLinWaves + wave; row < a.N;
       row += (int64_t)gridDim.x * kLinWaves) {
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    for (int l0 = 0; l0 < a.k; l0 += kLinWave) {
      SlotRound r;
      r.load(a.data, a.ds, a.sel, a.is, row, l0, lane, a.k, a.D);
      const int n = a.k - l0 < kLinWave ? a.k - l0 : kLinWave;
      // four slots in flight: their LDS reads are issued before the first multiply-add; a slot
      // past n reads the row of slot n - 1 and is not added
      for (int j = 0; j < n; j += kSlotsInFlight) {
        float v[kSlotsInFlight], x[kSlotsInFlight][C];
#pragma unroll
        for (int u = 0; u < kSlotsInFlight; ++u) {
          const int ju = j + u < n ? j + u : n - 1;
          v[u] = lane_value(r.v, ju);
          const float* t = mine + lane_value(r.s, ju) * MP;
#pragma unroll
          for (int c = 0; c < C; ++c) x[u][c] = t[c];
        }
#pragma unroll
        for (int u = 0; u < kSlotsInFlight; ++u)
#pragma unroll
          for (int c = 0; c < C; ++c)
            if (j + u < n) acc[c] = fmaf(v[u], x[u][c], acc[c]);  // wave-uniform
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (col0 + c < a.M) a.out[row * a.os + col0 + c] = a.bias ? acc[c] + b[c] : acc[c];
  }
}

// ----------------------------------------------------------------------- (B) sampled matmul
struct SampledArgs {
  const float* g;
  int64_t gs;
  const uint8_t* sel;
  int64_t is;
  const float* T;
  int64_t ts;
  float* dst;       // out, or with more than one panel the scratch [P][N, k]
  int64_t dstride;  // row stride of dst
  int64_t dpanel;   // floats between the panels of dst (0: one panel)
  int32_t N, D, k, M;
};

// The slot of a tile of R that lane `sub` < R holds after the reduce-scatter
template <int R>
__device__ __forceinline__ int held_slot(int sub) {
  int h = 0;
#pragma unroll
  for (int t = 0; (1 << t) < R; ++t) h |= ((sub >> t) & 1) * (R >> (t + 1));
  return h;
}

// Sums v[q] over the wave for every q < R: stage t halves the sums a lane holds and adds the
// partner's (lane ^ 2^t) terms of the half it keeps, which leaves one sum over R lanes; the
// strides R, 2 R, ... finish it. Every lane ends with the whole sum of slot held_slot(lane % R).
template <int R>
__device__ __forceinline__ float reduce_scatter(float (&v)[R], int lane) {
#pragma unroll
  for (int st = 0; (1 << st) < R; ++st) {
    const int half = R >> (st + 1);
    const bool up = (lane >> st) & 1;
#pragma unroll
    for (int q = 0; q < half; ++q) {
      const float send = up ? v[q] : v[q + half];
      const float keep = up ? v[q + half] : v[q];
      v[q] = keep + __shfl_xor(send, 1 << st, kLinWave);
    }
  }
  float tot = v[0];
#pragma unroll
  for (int m = R; m < kLinWave; m <<= 1) tot = tot + __shfl_xor(tot, m, kLinWave);
  return tot;
}

template <int MP>
__global__ __launch_bounds__(kLinThreads) void cbsr_sampled_kernel(const SampledArgs a) {
  extern __shared__ float lds[];  // T[:, panel], [D][MP]
  constexpr int C = MP / kLinWave, R = kLinSlotTile;
  const int lane = threadIdx.x & (kLinWave - 1), wave = wave_of_thread();
  const int p0 = blockIdx.y * MP, col0 = p0 + lane * C;
  stage_panel<MP>(lds, a.T, a.ts, a.D, a.M, p0);
  __syncthreads();

  const float* mine = lds + lane * C;
  float* dst = a.dst + (int64_t)blockIdx.y * a.dpanel;
  const int held = held_slot<R>(lane & (R - 1));

  for (int64_t row = (int64_t)blockIdx.x * kLinWaves + wave; row < a.N;
       row += (int64_t)gridDim.x * kLinWaves) {
    float gr[C];
#pragma unroll
    for (int c = 0; c < C; ++c) gr[c] = col0 + c < a.M ? a.g[row * a.gs + col0 + c] : 0.f;
    for (int l0 = 0; l0 < a.k; l0 += kLinWave) {
      SlotRound r;
      r.load(nullptr, 0, a.sel, a.is, row, l0, lane, a.k, a.D);
      const int n = a.k - l0 < kLinWave ? a.k - l0 : kLinWave;
      for (int t0 = 0; t0 < n; t0 += R) {
        float part[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
          part[q] = 0.f;
          if (t0 + q < n) {  // wave-uniform
            const float* t = mine + lane_value(r.s, t0 + q) * MP;
            float d = gr[0] * t[0];
#pragma unroll
            for (int c = 1; c < C; ++c) d = fmaf(gr[c], t[c], d);
            part[q] = d;
          }
        }
        const float tot = reduce_scatter<R>(part, lane);
        if (lane < R && t0 + held < n) dst[row * a.dstride + l0 + t0 + held] = tot;
      }
    }
  }
}

// out[n, l] = the panels' partial sums of (n, l), added in panel order
__global__ __launch_bounds__(256) void cbsr_sampled_sum_kernel(const float* __restrict__ part,
                                                               int32_t panels, int64_t count,
                                                               int32_t k, float* __restrict__ out,
                                                               int64_t os) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float v = part[i];
  for (int32_t p = 1; p < panels; ++p) v = v + part[(int64_t)p * count + i];
  out[(i / k) * os + i % k] = v;
}

// ------------------------------------------------------------------------- (C) weight grad
struct WeightGradArgs {
  const float* data;
  int64_t ds;
  const uint8_t* sel;
  int64_t is;
  const float* g;
  int64_t gs;
  float* part;   // [P][W][D, MP]
  float* psum;   // [W][D], or nullptr: no sums wanted
  int32_t N, D, k, M;
};

template <int MP>
__global__ __launch_bounds__(kLinThreads) void cbsr_weight_grad_kernel(const WeightGradArgs a) {
  extern __shared__ float lds[];  // the accumulator of dT[:, panel], [D][MP], then the sums [D]
  constexpr int C = MP / kLinWave;
  const int lane = threadIdx.x & (kLinWave - 1), wave = wave_of_thread();
  const int p0 = blockIdx.y * MP, col0 = p0 + lane * C;
  const int cells = a.D * MP;
  float* sums = lds + cells;
  const bool with_sums = a.psum != nullptr && blockIdx.y == 0;

  for (int i = threadIdx.x; i < cells + a.D; i += kLinThreads) lds[i] = 0.f;
  __syncthreads();

  float* mine = lds + lane * C;
  for (int64_t row = (int64_t)blockIdx.x * kLinWaves + wave; row < a.N;
       row += (int64_t)gridDim.x * kLinWaves) {
    float gr[C];
#pragma unroll
    for (int c = 0; c < C; ++c) gr[c] = col0 + c < a.M ? a.g[row * a.gs + col0 + c] : 0.f;
    for (int l0 = 0; l0 < a.k; l0 += kLinWave) {
      SlotRound r;
      r.load(a.data, a.ds, a.sel, a.is, row, l0, lane, a.k, a.D);
      const int n = a.k - l0 < kLinWave ? a.k - l0 : kLinWave;
      if (with_sums && lane < n) lds_add(sums + r.s, r.v);
      for (int j = 0; j < n; ++j) {
        const float v = lane_value(r.v, j);
        float* t = mine + lane_value(r.s, j) * MP;
#pragma unroll
        for (int c = 0; c < C; ++c)
          if (col0 + c < a.M) lds_add(t + c, v * gr[c]);
      }
    }
  }

  __syncthreads();
  float4* out = reinterpret_cast<float4*>(
      a.part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * cells);
  for (int i = threadIdx.x; i < cells / 4; i += kLinThreads)
    out[i] = reinterpret_cast<const float4*>(lds)[i];
  if (with_sums)
    for (int j = threadIdx.x; j < a.D; j += kLinThreads)
      a.psum[(int64_t)blockIdx.x * a.D + j] = sums[j];
}

// dT[j, col] and dsum[j] = the work-groups' partials, added in ascending order of the work-group.
// One thread per element of dT, then one per element of dsum.
__global__ __launch_bounds__(256) void cbsr_weight_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ psum, int32_t groups, int32_t mp,
    float* __restrict__ dT, int64_t dts, float* __restrict__ dsum, int32_t D, int32_t M) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t cells = (int64_t)D * M;
  if (i < cells) {
    const int j = (int)(i / M), col = (int)(i % M);
    const int64_t slab = (int64_t)D * mp;
    const float* p = part + (int64_t)(col / mp) * groups * slab + (int64_t)j * mp + col % mp;
    float v = 0.f;
    for (int32_t w = 0; w < groups; ++w) v = v + p[w * slab];
    dT[j * dts + col] = v;
  } else if (dsum && i < cells + D) {
    const int j = (int)(i - cells);
    float v = 0.f;
    for (int32_t w = 0; w < groups; ++w) v = v + psum[(int64_t)w * D + j];
    dsum[j] = v;
  }
}

// ------------------------------------------------------------------------------ entry points
// sizes and the strides of the CBSR tables shared by the three calls; strides are resolved (0: the
// row width)
static int check_shape(const std::string& w, int32_t N, int32_t D, int32_t k, int32_t M,
                       int64_t* ds, int64_t& is) {
  MAXK_CHECK_ARG(N >= 0 && M >= 1, w + "num_rows must be >= 0 and dim_m >= 1");
  if (D > maxk::kMaxDim) {
    set_error(w + "dim_origin above 256 is not supported (u8 selectors)");
    return MAXK_ERR_UNSUPPORTED;
  }
  MAXK_CHECK_ARG(k >= 1 && k <= D, w + "k must be between 1 and input dimension");
  if (panel_count(D, M) > kLinMaxPanels) {
    set_error(w + "dim_m beyond the grid's 65535 panels is not supported");
    return MAXK_ERR_UNSUPPORTED;
  }
  if (ds) {
    if (*ds == 0) *ds = k;
    MAXK_CHECK_ARG(*ds >= k, w + "data_stride must be >= k (0: k)");
  }
  if (is == 0) is = k;
  MAXK_CHECK_ARG(is >= k, w + "index_stride must be >= k (0: k)");
  return MAXK_OK;
}

// a [rows, width] array of `stride` elements per row: the bytes from its first to its last element
static int64_t span(int64_t rows, int64_t stride, int64_t width, int64_t elem) {
  return rows > 0 ? elem * ((rows - 1) * stride + width) : 0;
}

static int check_scratch(const std::string& w, const void* scratch, int64_t sbytes, int64_t need) {
  MAXK_CHECK_ARG(sbytes >= need, w + "scratch_bytes is below maxk_cbsr_linear_scratch_bytes");
  MAXK_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 15) == 0,
                 w + "scratch must be 16-B aligned");
  return MAXK_OK;
}

static int matmul(const float* data, int64_t ds, const uint8_t* sel, int64_t is, const float* T,
                  int64_t ts, const float* bias, float* out, int64_t os, int32_t N, int32_t D,
                  int32_t k, int32_t M, void* stream) {
  const std::string w("maxk_cbsr_matmul: ");
  int rc = check_shape(w, N, D, k, M, &ds, is);
  if (rc != MAXK_OK) return rc;
  if (ts == 0) ts = M;
  if (os == 0) os = M;
  MAXK_CHECK_ARG(ts >= M, w + "table_stride must be >= dim_m (0: dim_m)");
  MAXK_CHECK_ARG(os >= M, w + "out_stride must be >= dim_m (0: dim_m)");
  if (N == 0) return MAXK_OK;  // out has no element
  const Range ins[4] = {{data, span(N, ds, k, 4)}, {sel, span(N, is, k, 1)},
                        {T, span(D, ts, M, 4)}, {bias, bias ? 4 * (int64_t)M : 0}};
  const Range outs[1] = {{out, span(N, os, M, 4)}};
  rc = check_ranges(w, ins, 4, outs, 1);
  if (rc != MAXK_OK) return rc;
  const int64_t P = panel_count(D, M);
  const MatmulArgs a{data, ds, sel, is, T, ts, bias, out, os, N, D, k, M};
  if (int e = maxk::dispatch_variant(
          kMatmulVariants, select_matmul_variant(D, M), [&](auto i) -> int {
            constexpr int MP = kMatmulVariants[decltype(i)::value].mp;
            auto kern = cbsr_matmul_kernel<MP>;
            const size_t lds = sizeof(float) * (size_t)D * MP;
            if (lds > 64 * 1024) MAXK_HIP_TRY(allow_lds(kern, lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)row_groups(N, P), (unsigned)P),
                               dim3(kLinThreads), lds, (hipStream_t)stream, a);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_cbsr_matmul launch");
  return MAXK_OK;
}

static int sampled_matmul(const float* g, int64_t gs, const uint8_t* sel, int64_t is,
                          const float* T, int64_t ts, float* out, int64_t os, void* scratch,
                          int64_t sbytes, int32_t N, int32_t D, int32_t k, int32_t M,
                          void* stream) {
  const std::string w("maxk_cbsr_sampled_matmul: ");
  int rc = check_shape(w, N, D, k, M, nullptr, is);
  if (rc != MAXK_OK) return rc;
  if (gs == 0) gs = M;
  if (ts == 0) ts = M;
  if (os == 0) os = k;
  MAXK_CHECK_ARG(gs >= M, w + "g_stride must be >= dim_m (0: dim_m)");
  MAXK_CHECK_ARG(ts >= M, w + "table_stride must be >= dim_m (0: dim_m)");
  MAXK_CHECK_ARG(os >= k, w + "out_stride must be >= k (0: k)");
  const int64_t need = scratch_bytes(kLinSampled, N, D, k, M);
  rc = check_scratch(w, scratch, sbytes, need);
  if (rc != MAXK_OK) return rc;
  if (N == 0) return MAXK_OK;  // out has no element
  const Range ins[3] = {{g, span(N, gs, M, 4)}, {sel, span(N, is, k, 1)}, {T, span(D, ts, M, 4)}};
  const Range outs[2] = {{out, span(N, os, k, 4)}, {scratch, need}};
  rc = check_ranges(w, ins, 3, outs, 2);
  if (rc != MAXK_OK) return rc;
  const int64_t P = panel_count(D, M), count = (int64_t)N * k;
  const SampledArgs a{g, gs, sel, is, T, ts, P > 1 ? (float*)scratch : out, P > 1 ? k : os,
                      P > 1 ? count : 0, N, D, k, M};
  if (int e = maxk::dispatch_variant(
          kSampledVariants, select_sampled_variant(D, M), [&](auto i) -> int {
            constexpr int MP = kSampledVariants[decltype(i)::value].mp;
            auto kern = cbsr_sampled_kernel<MP>;
            const size_t lds = sizeof(float) * (size_t)D * MP;
            if (lds > 64 * 1024) MAXK_HIP_TRY(allow_lds(kern, lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)row_groups(N, P), (unsigned)P),
                               dim3(kLinThreads), lds, (hipStream_t)stream, a);
            return MAXK_OK;
          }))
    return e;
  if (P > 1)
    hipLaunchKernelGGL(cbsr_sampled_sum_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256),
                       0, (hipStream_t)stream, (const float*)scratch, (int32_t)P, count, k, out,
                       os);
  MAXK_LAUNCH_CHECK("maxk_cbsr_sampled_matmul launch");
  return MAXK_OK;
}

static int weight_grad(const float* data, int64_t ds, const uint8_t* sel, int64_t is,
                       const float* g, int64_t gs, float* dT, int64_t dts, float* dsum,
                       void* scratch, int64_t sbytes, int32_t N, int32_t D, int32_t k, int32_t M,
                       void* stream) {
  const std::string w("maxk_cbsr_weight_grad: ");
  int rc = check_shape(w, N, D, k, M, &ds, is);
  if (rc != MAXK_OK) return rc;
  if (gs == 0) gs = M;
  if (dts == 0) dts = M;
  MAXK_CHECK_ARG(gs >= M, w + "g_stride must be >= dim_m (0: dim_m)");
  MAXK_CHECK_ARG(dts >= M, w + "grad_table_stride must be >= dim_m (0: dim_m)");
  const int64_t need = scratch_bytes(kLinWeightGrad, N, D, k, M);
  rc = check_scratch(w, scratch, sbytes, need);
  if (rc != MAXK_OK) return rc;
  const Range ins[3] = {{data, span(N, ds, k, 4)}, {sel, span(N, is, k, 1)},
                        {g, span(N, gs, M, 4)}};
  const Range outs[3] = {{dT, span(D, dts, M, 4)}, {dsum, dsum ? 4 * (int64_t)D : 0},
                         {scratch, need}};
  rc = check_ranges(w, ins, 3, outs, 3);
  if (rc != MAXK_OK) return rc;
  const int64_t P = panel_count(D, M);
  const int32_t W = row_groups(N, P);
  const int mp = panel_width(D, M);
  float* part = (float*)scratch;
  float* psum = part + P * W * D * mp;
  if (N > 0) {
    const WeightGradArgs a{data, ds, sel, is, g, gs, part, dsum ? psum : nullptr, N, D, k, M};
    if (int e = maxk::dispatch_variant(
            kWeightGradVariants, select_weight_grad_variant(D, M), [&](auto i) -> int {
              constexpr int MP = kWeightGradVariants[decltype(i)::value].mp;
              auto kern = cbsr_weight_grad_kernel<MP>;
              const size_t lds = sizeof(float) * ((size_t)D * MP + D);
              if (lds > 64 * 1024) MAXK_HIP_TRY(allow_lds(kern, lds));
              hipLaunchKernelGGL(kern, dim3((unsigned)W, (unsigned)P), dim3(kLinThreads), lds,
                                 (hipStream_t)stream, a);
              return MAXK_OK;
            }))
      return e;
  }
  const int64_t threads = (int64_t)D * M + D;
  hipLaunchKernelGGL(cbsr_weight_reduce_kernel, dim3((unsigned)((threads + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, (const float*)part, (const float*)psum,
                     N > 0 ? W : 0, mp, dT, dts, dsum, D, M);
  MAXK_LAUNCH_CHECK("maxk_cbsr_weight_grad launch");
  return MAXK_OK;
}

}  // namespace maxk_lin

extern "C" int maxk_cbsr_matmul(const float* sp_data, int64_t data_stride, const uint8_t* sp_index,
                                int64_t index_stride, const float* table, int64_t table_stride,
                                const float* bias, float* out, int64_t out_stride,
                                int32_t num_rows, int32_t dim_origin, int32_t dim_k, int32_t dim_m,
                                void* stream) {
  return maxk_lin::matmul(sp_data, data_stride, sp_index, index_stride, table, table_stride, bias,
                          out, out_stride, num_rows, dim_origin, dim_k, dim_m, stream);
}

extern "C" int maxk_cbsr_sampled_matmul(const float* g, int64_t g_stride, const uint8_t* sp_index,
                                        int64_t index_stride, const float* table,
                                        int64_t table_stride, float* out, int64_t out_stride,
                                        void* scratch, int64_t scratch_bytes, int32_t num_rows,
                                        int32_t dim_origin, int32_t dim_k, int32_t dim_m,
                                        void* stream) {
  return maxk_lin::sampled_matmul(g, g_stride, sp_index, index_stride, table, table_stride, out,
                                  out_stride, scratch, scratch_bytes, num_rows, dim_origin, dim_k,
                                  dim_m, stream);
}

extern "C" int maxk_cbsr_weight_grad(const float* sp_data, int64_t data_stride,
                                     const uint8_t* sp_index, int64_t index_stride, const float* g,
                                     int64_t g_stride, float* grad_table,
                                     int64_t grad_table_stride, float* grad_sum, void* scratch,
                                     int64_t scratch_bytes, int32_t num_rows, int32_t dim_origin,
                                     int32_t dim_k, int32_t dim_m, void* stream) {
  return maxk_lin::weight_grad(sp_data, data_stride, sp_index, index_stride, g, g_stride,
                               grad_table, grad_table_stride, grad_sum, scratch, scratch_bytes,
                               num_rows, dim_origin, dim_k, dim_m, stream);
}

extern "C" int64_t maxk_cbsr_linear_scratch_bytes(int32_t op, int32_t num_rows, int32_t dim_origin,
                                                  int32_t dim_k, int32_t dim_m) {
  return maxk_lin::scratch_bytes(op, num_rows, dim_origin, dim_k, dim_m);
}

extern "C" int maxk_cbsr_linear_panel(int32_t dim_origin, int32_t dim_m, int32_t* out,
                                      int32_t capacity) {
  if (dim_origin < 1 || dim_origin > maxk::kMaxDim || dim_m < 1) return 0;
  const int64_t panels = maxk_lin::panel_count(dim_origin, dim_m);
  return maxk::copy_limits(out, capacity,
                           {maxk_lin::panel_width(dim_origin, dim_m),
                            (int32_t)(panels < INT32_MAX ? panels : INT32_MAX)});
}
