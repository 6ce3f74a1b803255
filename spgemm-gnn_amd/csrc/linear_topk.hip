// Fused linear + MaxK (include/maxk_hip.h, "Fused linear + MaxK"): for h [N, D_in], W [D, D_in]
//
//   y[n, :] = h[n, :] @ W.T + bias        (sp_data[n, :], sp_index[n, :]) = top-k of y[n, :]
//
// in one launch. The [N, D] pre-activation lives in matrix-core accumulators and, a few rows at a
// time, in LDS; HBM sees h once, the [N, k] tables and, if asked, the dense masked row.
//
// Work split. A work-group of 4 waves owns 64 consecutive rows and all DP >= D columns (DP = 64,
// 128 or 256: variants_linear_topk.h); a wave owns 16 of the rows and every column, so a row's
// top-k never leaves its wave. The product runs on v_mfma_f32_16x16x4_f32: a wave keeps DP / 16
// accumulator tiles of 16 x 16 (4 registers a lane each, 64 at DP = 256).
//
// Data movement. D_in is walked in chunks of KC = 32 columns. The 256 threads load the chunk of
// h [64][32] and of W [DP][32] with 16-byte loads (8 lanes cover a row's 128 bytes; scalar guarded
// loads where base, stride or the tail of D_in forbid them; rows past N, rows of W past D and
// columns past D_in are zeros) into registers while the matrix cores work on the chunk before,
// then store them into one LDS stage of [64 + DP] rows of 36 floats. The stage is single: a second
// one would take 90 KB at DP = 256 and leave one work-group a CU, where the register prefetch
// leaves three. A lane reads the stage 16 bytes at a time: lane (i, q) = (lane % 16, lane / 16)
// takes h[row i][kb + 4 q .. + 3], and W[column j][kb + 4 q .. + 3] for each column tile, which are
// the operands of four MFMA steps, step s multiplying over the depth {kb + 4 q + s : q = 0 .. 3}:
// the order of the sum over D_in differs from a dot product's, the set of its terms does not. The
// A operand of a step is read once and serves all DP / 16 column tiles. Rows of 36 floats put the
// 16 rows that a 16-byte read touches on 16 different bank groups.
//
// Epilogue. The bias is added to the accumulators. Register r of a lane's tile holds row
// 4 q + r, so the wave turns its rows round in four batches: batch r writes the four rows
// {r, 4 + r, 8 + r, 12 + r} row-major into its own LDS (4 x (DP + 16) floats, in the bytes of
// the stage, which the last barrier has retired), reads each row back as the top-k holds it (lane
// l: features 4 l .. 4 l + 3) and runs the exact selection and the emission of topk_select.h on it:
// the code of maxk_topk_cbsr, so the ties, the NaN rule and the dense masked row are its own.
//
// No scratch, no plan, no global atomics; one launch, capturable; every array takes a row stride.
#include "common.h"
#include "topk_select.h"
#include "variants_linear_topk.h"

namespace maxk_lt {

using maxk::check_ranges;
using maxk::DenseArg;
using maxk::Range;
using maxk::set_error;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Args {
  const float* h;
  int64_t hs;
  const float* W;
  int64_t ws;
  const float* bias;  // may be null
  float* sp_data;
  uint8_t* sp_index;
  int32_t ds, is;
  int32_t N, D_in, D, k;
};

// Columns col .. col + 3 of a row of `width` columns, zeros past it and for a row that is off
__device__ __forceinline__ float4 load_chunk4(const float* __restrict__ row, int col, int width,
                                              bool on, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on) {
    if (vec && col + 3 < width) {
      v = *reinterpret_cast<const float4*>(row + col);
    } else {
      if (col < width) v.x = row[col];
      if (col + 1 < width) v.y = row[col + 1];
      if (col + 2 < width) v.z = row[col + 2];
      if (col + 3 < width) v.w = row[col + 3];
    }
  }
  return v;
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int DP, bool kDense>
__global__ __launch_bounds__(kLtThreads) void linear_topk_kernel(const Args a,
                                                                 const DenseArg<kDense> dense) {
  constexpr int T = DP / 16;                       // column tiles of a wave
  constexpr int P = (kLtTileRows + DP) / 32;       // 16-byte loads per thread and chunk
  constexpr int PH = kLtTileRows / 32;             // of which rows of h
  constexpr int S = kLtRowFloats;
  constexpr int ES = DP + kLtEpiPad;               // floats of a turned row
  static_assert(T % 4 == 0 && kLtChunk == 32 && kLtThreads == 256, "tile walk below");
  __shared__ __align__(16) unsigned char smem[lds_bytes(DP)];
  float* const h_l = reinterpret_cast<float*>(smem);
  float* const w_l = h_l + kLtTileRows * S;

  const int tid = threadIdx.x, lane = tid & (kLtWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kLtWave);
  const int i = lane & 15, q = lane >> 4;
  const int64_t row_blk = (int64_t)blockIdx.x * kLtTileRows;

  // this thread's part of a chunk: row lr (+ 32 p) of the stage, columns lc .. lc + 3
  const int lr = tid >> 3, lc = 4 * (tid & 7);
  const bool vec_h = ((reinterpret_cast<uintptr_t>(a.h) & 15) | (uintptr_t)(a.hs & 3)) == 0;
  const bool vec_w = ((reinterpret_cast<uintptr_t>(a.W) & 15) | (uintptr_t)(a.ws & 3)) == 0;
  const float* const h_row = a.h + (row_blk + lr) * a.hs;
  const float* const w_row = a.W + (int64_t)lr * a.ws;

  float4 pre[P];
  auto load = [&](int c) {
    const int col = c * kLtChunk + lc;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (p < PH)
        pre[p] = load_chunk4(h_row + (int64_t)(32 * p) * a.hs, col, a.D_in,
                             row_blk + lr + 32 * p < a.N, vec_h);
      else
        pre[p] = load_chunk4(w_row + (int64_t)(32 * (p - PH)) * a.ws, col, a.D_in,
                             lr + 32 * (p - PH) < a.D, vec_w);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int p = 0; p < P; ++p)
      *reinterpret_cast<float4*>(h_l + (lr + 32 * p) * S + lc) = pre[p];  // w_l follows h_l
  };

  f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int chunks = (a.D_in + kLtChunk - 1) / kLtChunk;
  load(0);
  store();
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    const bool more = c + 1 < chunks;  // uniform
    if (more) load(c + 1);
    const float* const ar = h_l + (wave * kLtWaveRows + i) * S + 4 * q;
    const float* const br = w_l + i * S + 4 * q;
#pragma unroll
    for (int kb = 0; kb < kLtChunk; kb += 16) {
      const float4 av = *reinterpret_cast<const float4*>(ar + kb);
#pragma unroll
      for (int t0 = 0; t0 < T; t0 += 4) {
        float4 bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          bv[u] = *reinterpret_cast<const float4*>(br + (t0 + u) * 16 * S + kb);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[t0 + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv[u].x, acc[t0 + u], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[t0 + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv[u].y, acc[t0 + u], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[t0 + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv[u].z, acc[t0 + u], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
          acc[t0 + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv[u].w, acc[t0 + u], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave has read the stage
    if (more) {
      store();
      __syncthreads();
    }
  }

  const int64_t row0 = row_blk + wave * kLtWaveRows;
  if (row0 >= a.N) return;  // wave-uniform, behind the last barrier
  if (a.bias) {             // uniform
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int col = 16 * t + i;
      const float b = col < a.D ? a.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] = __fadd_rn(acc[t][r], b);
    }
  }

  // the stage is retired: this wave's turned rows, histogram and emission rows in its place
  unsigned char* const mine = smem + wave * wave_epilogue_bytes(DP);
  float* const tile = reinterpret_cast<float*>(mine);
  uint32_t* const hist = reinterpret_cast<uint32_t*>(tile + kLtEpiRows * ES);
  float* const stage_v = reinterpret_cast<float*>(hist + 256);
  uint8_t* const stage_i = reinterpret_cast<uint8_t*>(stage_v + 256);
  bool valid[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) valid[e] = 4 * lane + e < a.D;
#pragma unroll 1
  for (int r = 0; r < 4; ++r) {
    // rows 4 q + r of the wave, q = 0 .. 3: lane (i, q) holds columns 16 t + i of row 4 q + r
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float v = r == 0 ? acc[t][0] : r == 1 ? acc[t][1] : r == 2 ? acc[t][2] : acc[t][3];
      tile[q * ES + 16 * t + i] = v;
    }
    wave_lds_fence();
#pragma unroll 1
    for (int q2 = 0; q2 < kLtEpiRows; ++q2) {
      if (row0 + 4 * q2 + r >= a.N) continue;  // wave-uniform
      const int row = (int)(row0 + 4 * q2 + r);
      float x[4] = {0.f, 0.f, 0.f, 0.f};
      if (4 * lane < DP) {
        const float4 v = *reinterpret_cast<const float4*>(tile + q2 * ES + 4 * lane);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
      }
      bool sel[4];
      maxk::exact_select(x, valid, a.k, hist, lane, sel);
      if (a.k > kLtWave)  // uniform
        maxk::emit_staged<true, kDense, false, kDense>(x, sel, lane, row, a.k, stage_v, stage_i,
                                                       a.sp_data, a.sp_index, a.ds, a.is, nullptr,
                                                       maxk::TopkRec{}, maxk::DropArg<false>{},
                                                       dense, a.D);
      else
        maxk::emit_staged<false, kDense, false, kDense>(x, sel, lane, row, a.k, stage_v, stage_i,
                                                        a.sp_data, a.sp_index, a.ds, a.is, nullptr,
                                                        maxk::TopkRec{}, maxk::DropArg<false>{},
                                                        dense, a.D);
    }
    wave_lds_fence();  // the next batch overwrites the turned rows
  }
}

// a [rows, width] array of `stride` elements per row: the bytes from its first to its last element
static int64_t span(int64_t rows, int64_t stride, int64_t width, int64_t elem) {
  return rows > 0 ? elem * ((rows - 1) * stride + width) : 0;
}

static int linear_topk(const float* h, int64_t hs, const float* W, int64_t ws, const float* bias,
                       int32_t N, int32_t D_in, int32_t D, int32_t k, float* sp_data, int64_t ds,
                       uint8_t* sp_index, int64_t is, float* dense, int64_t dstride,
                       void* stream) {
  const std::string w("maxk_linear_topk: ");
  MAXK_CHECK_ARG(N >= 0 && D_in >= 1, w + "num_rows must be >= 0 and dim_in >= 1");
  if (D > maxk::kMaxDim) {
    set_error(w + "dim_origin above 256 is not supported (u8 selectors)");
    return MAXK_ERR_UNSUPPORTED;
  }
  MAXK_CHECK_ARG(k >= 1 && k <= D, w + "k must be between 1 and input dimension");
  if (hs == 0) hs = D_in;
  if (ws == 0) ws = D_in;
  if (ds == 0) ds = k;
  if (is == 0) is = k;
  if (dstride == 0) dstride = D;
  MAXK_CHECK_ARG(hs >= D_in, w + "h_stride must be >= dim_in (0: dim_in)");
  MAXK_CHECK_ARG(ws >= D_in, w + "w_stride must be >= dim_in (0: dim_in)");
  MAXK_CHECK_ARG(ds >= k && ds <= INT32_MAX / 4, w + "data_stride must be >= k (0: k)");
  MAXK_CHECK_ARG(is >= k && is <= INT32_MAX, w + "index_stride must be >= k (0: k)");
  MAXK_CHECK_ARG(!dense || dstride >= D,
                 w + "dense_stride must be >= dim_origin (0: dim_origin)");
  if (N == 0) return MAXK_OK;  // no row, no output element
  const Range ins[3] = {{h, span(N, hs, D_in, 4)}, {W, span(D, ws, D_in, 4)},
                        {bias, bias ? 4 * (int64_t)D : 0}};
  const Range outs[3] = {{sp_data, span(N, ds, k, 4)}, {sp_index, span(N, is, k, 1)},
                         {dense, dense ? span(N, dstride, D, 4) : 0}};
  if (int rc = check_ranges(w, ins, 3, outs, 3)) return rc;
  const Args a{h, hs, W, ws, bias, sp_data, sp_index, (int32_t)ds, (int32_t)is, N, D_in, D, k};
  const unsigned grid = (unsigned)(((int64_t)N + kLtTileRows - 1) / kLtTileRows);
  if (int e = maxk::dispatch_variant(
          kLinearTopkVariants, select_linear_topk_variant(D, dense != nullptr),
          [&](auto idx) -> int {
            constexpr LinearTopkVariant V = kLinearTopkVariants[decltype(idx)::value];
            DenseArg<V.dense> dn;
            if constexpr (V.dense) dn = DenseArg<true>{dense, dstride};
            hipLaunchKernelGGL((linear_topk_kernel<V.dp, V.dense>), dim3(grid), dim3(kLtThreads),
                               0, (hipStream_t)stream, a, dn);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_linear_topk launch");
  return MAXK_OK;
}

}  // namespace maxk_lt

extern "C" int maxk_linear_topk(const float* h, int64_t h_stride, const float* weight,
                                int64_t w_stride, const float* bias, int32_t num_rows,
                                int32_t dim_in, int32_t dim_origin, int32_t dim_k, float* sp_data,
                                int64_t data_stride, uint8_t* sp_index, int64_t index_stride,
                                float* dense, int64_t dense_stride, void* stream) {
  return maxk_lt::linear_topk(h, h_stride, weight, w_stride, bias, num_rows, dim_in, dim_origin,
                              dim_k, sp_data, data_stride, sp_index, index_stride, dense,
                              dense_stride, stream);
}

extern "C" int maxk_linear_topk_tile(int32_t dim_origin, int32_t* out, int32_t capacity) {
  if (dim_origin < 1 || dim_origin > maxk::kMaxDim) return 0;
  const int dp = maxk_lt::padded_dim(dim_origin);
  return maxk::copy_limits(out, capacity,
                           {maxk_lt::kLtTileRows, dp, maxk_lt::kLtChunk, maxk_lt::lds_bytes(dp)});
}
