// Fused linear + MaxK on 16-bit operands (include/maxk_hip.h, "Fused linear + MaxK, 16-bit
// operands"): for h [N, D_in] and W [D, D_in], both bf16 or both f16, and an f32 bias
//
//   y[n, :] = h[n, :] @ W.T + bias        (sp_data[n, :], sp_index[n, :]) = top-k of y[n, :]
//
// in one launch. The products of two 16-bit values are exact in f32 and the sums are f32 in the
// matrix-core accumulators; the [N, D] pre-activation is never written, the tables and the dense
// masked row are f32 as everywhere else in the library.
//
// Work split. A work-group of 8 waves owns 128 consecutive rows and all DP >= D columns (DP = 64,
// 128 or 256: variants_linear_topk16.h); a wave owns 16 of the rows and every column, so a row's
// top-k never leaves its wave. The product runs on v_mfma_f32_16x16x32_bf16 / _f16: a wave keeps
// DP / 16 accumulator tiles of 16 x 16 (4 registers a lane each, 64 at DP = 256), and one
// instruction covers a depth of 32 where the f32 kernel's covers 4. With the arithmetic an eighth
// of the f32 kernel's, what a row costs is the traffic of W into and out of LDS: 128 rows a
// work-group halve the chunks of W that are loaded and stored per row of h, and two work-groups
// of 8 waves a CU (4 waves a SIMD, at most 128 registers) let one stream h while the other
// selects.
//
// W is not resident. The whole of a bf16 W [256, 256] with padding is 132 KB: one work-group a CU,
// no overlap of one group's epilogue with another's product, and a limit on D_in that the entry
// point does not have. A chunk of W [DP][64] is 32 KB from L2, shared by 128 rows.
//
// Data movement. D_in is walked in chunks of KC = 64 elements, 128 bytes a row. The 512 threads
// load the chunk of h [128][64] and of W [DP][64] with 16-byte loads (8 lanes cover a row's 128
// bytes; guarded 2-byte loads where base, stride or the tail of D_in forbid them, so a row may
// start on any 2-byte boundary; rows past N, rows of W past D and depth past D_in are zeros) into
// registers while the matrix cores work on the chunk before, then store them into one LDS stage of
// [128 + DP] rows of 72 elements (36 words: the 16 rows that a 16-byte read touches fall on 16
// different bank groups). Lane (i, q) = (lane % 16, lane / 16) reads h[row i][kb + 8 q .. + 7] and,
// for each column tile, W[column j][kb + 8 q .. + 7], one ds_read_b128 each and the whole operand
// of one MFMA; the A operand is read once per step and serves all DP / 16 column tiles. A chunk is
// two steps a column tile, between one pair of barriers.
//
// Epilogue. As linear_topk.hip: the accumulator layout is that of the 16x16x4 f32 instruction
// (register r of a lane's tile is row 4 q + r, column i), so the bias is added in registers and the
// wave turns its rows round in four batches through its own LDS (in the bytes of the stage, which
// the last barrier has retired), reads each row back as the top-k holds it and runs exact_select
// and emit_staged of topk_select.h on it: ties, the NaN rule and the dense masked row are those of
// maxk_topk_cbsr.
//
// No scratch, no plan, no global atomics; one launch, capturable; every array takes a row stride.
#include "common.h"
#include "topk_select.h"
#include "variants_linear_topk16.h"

namespace maxk_lt16 {

using maxk::check_ranges;
using maxk::DenseArg;
using maxk::Range;
using maxk::set_error;

static_assert(kBf16 == MAXK_DTYPE_BF16 && kF16 == MAXK_DTYPE_F16, "the table's dtype codes");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct Args {
  const uint16_t* h;  // bits of bf16 or f16
  int64_t hs;
  const uint16_t* W;
  int64_t ws;
  const float* bias;  // may be null
  float* sp_data;
  uint8_t* sp_index;
  int32_t ds, is;
  int32_t N, D_in, D, k;
};

// Elements col .. col + 7 of a row of `width` elements, zeros past it and for a row that is off
__device__ __forceinline__ uint4 load_chunk8(const uint16_t* __restrict__ row, int col, int width,
                                             bool on, bool vec) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (on) {
    if (vec && col + 7 < width) {
      v = *reinterpret_cast<const uint4*>(row + col);
    } else {
      uint32_t e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = col + j < width ? (uint32_t)row[col + j] : 0u;
      v = make_uint4(e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16);
    }
  }
  return v;
}

// One step of depth 32 on a column tile: the 16 bytes of each operand are the lane's 8 elements
template <int kDtype>
__device__ __forceinline__ f32x4 mfma_step(const uint4& a, const uint4& b, const f32x4& c) {
  if constexpr (kDtype == kBf16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 4 waves a SIMD: two work-groups a CU, so at most 128 registers a lane
template <int DP, bool kDense, int kDtype>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void linear_topk16_kernel(const Args a, const DenseArg<kDense> dense) {
  constexpr int T = DP / 16;                        // column tiles of a wave
  constexpr int P = (kTileRows + DP) / kLoadRows;   // 16-byte loads per thread and chunk
  constexpr int PH = kTileRows / kLoadRows;         // of which rows of h
  constexpr int S = kRowElems;
  constexpr int ES = DP + kEpiPad;                  // floats of a turned row
  static_assert(T % 4 == 0 && kChunk == 2 * kStep && kThreads == 512, "tile walk below");
  __shared__ __align__(16) unsigned char smem[lds_bytes(DP)];
  uint16_t* const h_l = reinterpret_cast<uint16_t*>(smem);
  uint16_t* const w_l = h_l + kTileRows * S;

  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int i = lane & 15, q = lane >> 4;
  const int64_t row_blk = (int64_t)blockIdx.x * kTileRows;

  // this thread's part of a chunk: row lr (+ 64 p) of the stage, elements lc .. lc + 7
  const int lr = tid >> 3, lc = 8 * (tid & 7);
  const bool vec_h = ((reinterpret_cast<uintptr_t>(a.h) & 15) | (uintptr_t)(a.hs & 7)) == 0;
  const bool vec_w = ((reinterpret_cast<uintptr_t>(a.W) & 15) | (uintptr_t)(a.ws & 7)) == 0;
  const uint16_t* const h_row = a.h + (row_blk + lr) * a.hs;
  const uint16_t* const w_row = a.W + (int64_t)lr * a.ws;

  uint4 pre[P];
  auto load = [&](int c) {
    const int col = c * kChunk + lc;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (p < PH)
        pre[p] = load_chunk8(h_row + (int64_t)(kLoadRows * p) * a.hs, col, a.D_in,
                             row_blk + lr + kLoadRows * p < a.N, vec_h);
      else
        pre[p] = load_chunk8(w_row + (int64_t)(kLoadRows * (p - PH)) * a.ws, col, a.D_in,
                             lr + kLoadRows * (p - PH) < a.D, vec_w);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int p = 0; p < P; ++p)
      *reinterpret_cast<uint4*>(h_l + (lr + kLoadRows * p) * S + lc) = pre[p];  // w_l follows h_l
  };

  f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int chunks = (a.D_in + kChunk - 1) / kChunk;
  load(0);
  store();
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    const bool more = c + 1 < chunks;  // uniform
    if (more) load(c + 1);
    const uint16_t* const ar = h_l + (wave * kWaveRows + i) * S + 8 * q;
    const uint16_t* const br = w_l + i * S + 8 * q;
#pragma unroll
    for (int kb = 0; kb < kChunk; kb += kStep) {
      const uint4 av = *reinterpret_cast<const uint4*>(ar + kb);
#pragma unroll
      for (int t0 = 0; t0 < T; t0 += 4) {
        uint4 bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          bv[u] = *reinterpret_cast<const uint4*>(br + (t0 + u) * 16 * S + kb);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t0 + u] = mfma_step<kDtype>(av, bv[u], acc[t0 + u]);
      }
    }
    __syncthreads();  // every wave has read the stage
    if (more) {
      store();
      __syncthreads();
    }
  }

  const int64_t row0 = row_blk + wave * kWaveRows;
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
  uint32_t* const hist = reinterpret_cast<uint32_t*>(tile + kEpiRows * ES);
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
    for (int q2 = 0; q2 < kEpiRows; ++q2) {
      if (row0 + 4 * q2 + r >= a.N) continue;  // wave-uniform
      const int row = (int)(row0 + 4 * q2 + r);
      float x[4] = {0.f, 0.f, 0.f, 0.f};
      if (4 * lane < DP) {
        const float4 v = *reinterpret_cast<const float4*>(tile + q2 * ES + 4 * lane);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
      }
      bool sel[4];
      maxk::exact_select(x, valid, a.k, hist, lane, sel);
      if (a.k > kWave)  // uniform
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

static int linear_topk16(const void* h, int64_t hs, const void* W, int64_t ws, const float* bias,
                         int32_t dtype, int32_t N, int32_t D_in, int32_t D, int32_t k,
                         float* sp_data, int64_t ds, uint8_t* sp_index, int64_t is, float* dense,
                         int64_t dstride, void* stream) {
  const std::string w("maxk_linear_topk_16: ");
  MAXK_CHECK_ARG(dtype == MAXK_DTYPE_BF16 || dtype == MAXK_DTYPE_F16,
                 w + "dtype must be MAXK_DTYPE_BF16 or MAXK_DTYPE_F16");
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
  const Range ins[3] = {{h, span(N, hs, D_in, 2)}, {W, span(D, ws, D_in, 2)},
                        {bias, bias ? 4 * (int64_t)D : 0}};
  const Range outs[3] = {{sp_data, span(N, ds, k, 4)}, {sp_index, span(N, is, k, 1)},
                         {dense, dense ? span(N, dstride, D, 4) : 0}};
  if (int rc = check_ranges(w, ins, 3, outs, 3)) return rc;
  const Args a{static_cast<const uint16_t*>(h), hs, static_cast<const uint16_t*>(W), ws, bias,
               sp_data, sp_index, (int32_t)ds, (int32_t)is, N, D_in, D, k};
  const unsigned grid = (unsigned)(((int64_t)N + kTileRows - 1) / kTileRows);
  if (int e = maxk::dispatch_variant(
          kLinearTopk16Variants, select_linear_topk16_variant(D, dense != nullptr, dtype),
          [&](auto idx) -> int {
            constexpr LinearTopk16Variant V = kLinearTopk16Variants[decltype(idx)::value];
            DenseArg<V.dense> dn;
            if constexpr (V.dense) dn = DenseArg<true>{dense, dstride};
            hipLaunchKernelGGL((linear_topk16_kernel<V.dp, V.dense, V.dtype>), dim3(grid),
                               dim3(kThreads), 0, (hipStream_t)stream, a, dn);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_linear_topk_16 launch");
  return MAXK_OK;
}

}  // namespace maxk_lt16

extern "C" int maxk_linear_topk_16(const void* h, int64_t h_stride, const void* weight,
                                   int64_t w_stride, const float* bias, int32_t dtype,
                                   int32_t num_rows, int32_t dim_in, int32_t dim_origin,
                                   int32_t dim_k, float* sp_data, int64_t data_stride,
                                   uint8_t* sp_index, int64_t index_stride, float* dense,
                                   int64_t dense_stride, void* stream) {
  return maxk_lt16::linear_topk16(h, h_stride, weight, w_stride, bias, dtype, num_rows, dim_in,
                                  dim_origin, dim_k, sp_data, data_stride, sp_index, index_stride,
                                  dense, dense_stride, stream);
}

extern "C" int maxk_linear_topk_16_tile(int32_t dim_origin, int32_t* out, int32_t capacity) {
  if (dim_origin < 1 || dim_origin > maxk::kMaxDim) return 0;
  const int dp = maxk_lt16::padded_dim(dim_origin);
  return maxk::copy_limits(
      out, capacity, {maxk_lt16::kTileRows, dp, maxk_lt16::kChunk, maxk_lt16::lds_bytes(dp)});
}
