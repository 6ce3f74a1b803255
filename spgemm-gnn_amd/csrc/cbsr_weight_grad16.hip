// Weight and bias gradient of the 16-bit fused linear + MaxK (include/maxk_hip.h, "MaxK linear
// layers, 16-bit weight gradient"): with the CBSR tables v [N, k] f32 and s [N, k] u8 and a bf16 or
// f16 g [N, M],
//
//   vr       = v rounded to the type of g
//   dT[j, :] = sum_{(n, l): s[n, l] = j} vr[n, l] g[n, :]      dsum[j] = sum of the same vr[n, l]
//
// as the dense-shaped product dT [D, M] = A^T B on the matrix cores, with A = densify(vr) [N, D]
// and B = g, reduced over N. The densified rows are mostly zeros, which costs arithmetic that
// v_mfma_f32_16x16x32_bf16 / _f16 has to spare, and buys a kernel without LDS atomics or a sort
// whose summation order is fixed: the call repeats bit for bit, which cbsr_linear.hip's (C) does
// not. A is never in memory: it is built, 64 rows at a time, in LDS.
//
// Work split. A work-group of 8 waves owns one panel of MP = 128 or 64 columns of M (blockIdx.y) and
// a contiguous range of 64-row chunks (blockIdx.x); all panels together are at most kGroups
// work-groups. It keeps the whole [DP, MP] accumulator of its panel in registers, DP = D rounded up
// to 64, 128 or 256: the waves are WF groups along the features times WC along the columns
// (8 x 1, at DP = 64 4 x 2), a wave holds RT x CT tiles of 16 x 16 (2 x 8 at DP = 256, MP = 128:
// 64 registers a lane) and, in the first panel, RT tiles more that multiply A^T by a column of
// ones: dsum, at an eighth more instructions in that panel and in the same fixed order.
//
// Data movement, per chunk of 64 rows (two MFMA depths of 32), between two barriers:
//   * The 512 threads load the chunk of g [64][MP] with 16-byte loads (guarded 2-byte loads where
//     base, stride or the tail of M forbid them; rows past N and columns past M are zeros) and the
//     rows' slots (8 threads a row, slot l0 + 8 j: value rounded and packed with its selector, 8
//     registers for k <= 64; slots past 64 are read again when they are used) into registers while
//     the matrix cores work on the chunk before.
//   * g goes to LDS as it is, row-major [64][MP + 16]. The B operand of the MFMA is 8 consecutive
//     rows of one column: ds_read_b64_tr_b16 delivers four of them a read (in a group of 16 lanes,
//     lane l reads the 8 bytes at row l / 4, columns 4 (l % 4) ...; lane i receives column i of
//     those four rows), so two reads are one operand and no transposed copy of g is ever stored.
//   * A^T [DP][64 + 8] lives in LDS, zeroed once. A slot writes its rounded value at
//     [s][position of its row] with one 2-byte store, and after the chunk's MFMAs the same thread
//     writes zero there again: k stores a row each way instead of a clear of the tile. The rows of
//     a 32-row step are permuted over its depth positions (depth_position, variants_weight_grad16.h)
//     so that lane (i, q) reads its 8 positions of feature i with one ds_read_b128 while the two
//     transposing reads take rows 4 q ... and 16 + 4 q ..., 16 different rows a read.
//   A thread's rows of the slot pass stay in its wave, and a wave's LDS operations keep their order,
//   so the zeros of one chunk and the values of the next need no barrier between them.
//
// Reduction. A work-group leaves its accumulator in scratch, [P][W][D, MP] and [W][D], and a second
// kernel adds the W partials in ascending order and writes every element of dT and dsum.
//
// No plan, no global atomics, nothing allocated, capturable; every array takes a row stride.
#include "common.h"
#include "variants_weight_grad16.h"

namespace maxk_wg16 {

using maxk::check_ranges;
using maxk::Range;
using maxk::set_error;

static_assert(kBf16 == MAXK_DTYPE_BF16 && kF16 == MAXK_DTYPE_F16, "the table's dtype codes");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));

struct Args {
  const float* data;
  int64_t ds;
  const uint8_t* sel;
  int64_t is;
  const uint16_t* g;  // bits of bf16 or f16
  int64_t gs;
  float* part;        // [P][W][D, MP]
  float* psum;        // [W][D], or nullptr: no sums wanted
  int32_t N, D, k, M;
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

// The bits of x rounded to the type, to nearest even: torch's .to(dtype), its NaN included
template <int kDtype>
__device__ __forceinline__ uint32_t round16(float x) {
  if constexpr (kDtype == kBf16) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  } else {
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x);  // v_cvt_f16_f32: overflow is Inf
  }
}

template <int kDtype>
__device__ __forceinline__ f32x4 mfma_step(const uint4& a, const uint4& b, const f32x4& c) {
  if constexpr (kDtype == kBf16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ds_read_b64_tr_b16 at p (LDS, 8-byte aligned): four rows of this lane's column
__device__ __forceinline__ uint2 read_transposed(const uint16_t* p) {
  typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
  return __builtin_bit_cast(
      uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)const_cast<uint16_t*>(p)));
}

// 4 waves a SIMD: two work-groups a CU, so at most 128 registers a lane
template <int DP, int MP, int kDtype>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void weight_grad16_kernel(const Args a) {
  constexpr int WF = waves_along_features(DP), WC = kWaves / WF;
  constexpr int RT = DP / 16 / WF, CT = MP / 16 / WC;  // a wave's tiles: features x columns
  constexpr int GS = MP + kGPad;                       // elements of a staged row of g
  constexpr int LPR = MP / 8;                          // 16-byte loads a row of the panel
  constexpr int GR = kThreads / LPR;                   // rows one round of loads covers
  constexpr int GP = kChunkRows / GR;                  // rounds a chunk
  static_assert(kChunkRows == 2 * kStep && kThreads == kChunkRows * kSlotLanes && GP >= 1 &&
                (2 * GS) % 16 == 0, "chunk walk below");
  __shared__ __align__(16) uint16_t smem[lds_bytes(DP, MP) / 2];
  uint16_t* const at = smem;               // A^T [DP][kARow]
  uint16_t* const gl = smem + DP * kARow;  // g [64][GS]

  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int i = lane & 15, q = lane >> 4;
  const int wf = wave % WF, wc = wave / WF;
  const int p0 = blockIdx.y * MP, W = gridDim.x;
  const int64_t chunks = ((int64_t)a.N + kChunkRows - 1) / kChunkRows;
  const int64_t c_begin = chunks * blockIdx.x / W, c_end = chunks * (blockIdx.x + 1) / W;
  const bool with_sum = a.psum != nullptr && blockIdx.y == 0 && wc == 0;  // wave-uniform

  // this thread's part of the slot pass: row srow of the chunk, slots sl, sl + 8, ...
  const int srow = tid / kSlotLanes, sl = tid % kSlotLanes;
  uint16_t* const at_mine = at + ((srow & ~(kStep - 1)) | depth_position(srow & (kStep - 1)));
  auto selector = [&](int64_t row, int l) -> uint32_t {  // clamped into [0, D)
    const int raw = a.sel[row * a.is + l];
    return raw < a.D ? raw : a.D - 1;
  };
  // and of the chunk of g: rows grow (+ GR p), elements gcol .. gcol + 7 of the panel
  const int grow = tid / LPR, gcol = 8 * (tid % LPR);
  const bool vec = ((reinterpret_cast<uintptr_t>(a.g) & 15) | (uintptr_t)(a.gs & 7)) == 0;

  // the first 8 slots of the thread: rounded values two a register, selectors four a register;
  // slots that are not there (past k, rows past N) are zeros and are not stored
  uint32_t pre_v[kSlotsHeld / 2], pre_s[kSlotsHeld / 4], cur_s[kSlotsHeld / 4];
  uint4 gpre[GP];
  auto load = [&](int64_t c) {
    const int64_t r0 = c * kChunkRows, row = r0 + srow;
#pragma unroll
    for (int j = 0; j < kSlotsHeld; ++j) {
      const int l = sl + kSlotLanes * j;
      const bool on = row < a.N && l < a.k;
      const uint32_t v = on ? round16<kDtype>(a.data[row * a.ds + l]) : 0u;
      const uint32_t s = on ? selector(row, l) : 0u;
      pre_v[j / 2] = j % 2 ? pre_v[j / 2] | v << 16 : v;
      pre_s[j / 4] = j % 4 ? pre_s[j / 4] | s << 8 * (j % 4) : s;
    }
#pragma unroll
    for (int p = 0; p < GP; ++p) {
      const int64_t grow_p = r0 + grow + GR * p;
      const bool on = grow_p < a.N;
      gpre[p] = load_chunk8(a.g + (on ? grow_p : 0) * a.gs, p0 + gcol, a.M, on, vec);
    }
  };
  // the chunk into LDS: g as it is, a slot's value at [selector][position of the row]
  auto stage = [&](int64_t c) {
#pragma unroll
    for (int p = 0; p < GP; ++p)
      *reinterpret_cast<uint4*>(gl + (grow + GR * p) * GS + gcol) = gpre[p];
    const int64_t row = c * kChunkRows + srow;
    if (row >= a.N) return;
#pragma unroll
    for (int j = 0; j < kSlotsHeld; ++j) {
      cur_s[j / 4] = pre_s[j / 4];
      if (sl + kSlotLanes * j < a.k)
        at_mine[(pre_s[j / 4] >> 8 * (j % 4) & 0xffu) * kARow] =
            (uint16_t)(pre_v[j / 2] >> 16 * (j % 2));
    }
    for (int l = sl + kSlotLanes * kSlotsHeld; l < a.k; l += kSlotLanes)  // k > 64
      at_mine[selector(row, l) * kARow] = (uint16_t)round16<kDtype>(a.data[row * a.ds + l]);
  };
  // zeros again where the chunk's slots wrote, behind its MFMAs
  auto clear = [&](int64_t c) {
    const int64_t row = c * kChunkRows + srow;
    if (row >= a.N) return;
#pragma unroll
    for (int j = 0; j < kSlotsHeld; ++j)
      if (sl + kSlotLanes * j < a.k) at_mine[(cur_s[j / 4] >> 8 * (j % 4) & 0xffu) * kARow] = 0;
    for (int l = sl + kSlotLanes * kSlotsHeld; l < a.k; l += kSlotLanes)
      at_mine[selector(row, l) * kARow] = 0;
  };

  f32x4 acc[RT][CT], sum[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    sum[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // the B operand of the sums: column 0 of its tile is ones, the others zeros
  const uint32_t one2 = i == 0 ? (kDtype == kBf16 ? 0x3f803f80u : 0x3c003c00u) : 0u;
  const uint4 ones = make_uint4(one2, one2, one2, one2);

  for (int e = tid; e < DP * kARow / 8; e += kThreads)
    reinterpret_cast<uint4*>(at)[e] = make_uint4(0u, 0u, 0u, 0u);
  if (c_begin < c_end) load(c_begin);
  __syncthreads();  // A^T is zeros

  const uint16_t* const ar = at + (wf * RT * 16 + i) * kARow + 8 * q;
  const uint16_t* const br = gl + (4 * q + (i >> 2)) * GS + wc * CT * 16 + 4 * (i & 3);
  for (int64_t c = c_begin; c < c_end; ++c) {
    stage(c);
    __syncthreads();
    if (c + 1 < c_end) load(c + 1);  // uniform
#pragma unroll
    for (int kb = 0; kb < kChunkRows; kb += kStep) {
      uint4 av[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        av[rt] = *reinterpret_cast<const uint4*>(ar + rt * 16 * kARow + kb);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const uint2 lo = read_transposed(br + kb * GS + ct * 16);               // rows 4 q ...
        const uint2 hi = read_transposed(br + (kb + kStep / 2) * GS + ct * 16);  // 16 + 4 q ...
        const uint4 bv = make_uint4(lo.x, lo.y, hi.x, hi.y);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][ct] = mfma_step<kDtype>(av[rt], bv, acc[rt][ct]);
      }
      if (with_sum) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) sum[rt] = mfma_step<kDtype>(av[rt], ones, sum[rt]);
      }
    }
    __syncthreads();  // every wave has read the chunk
    clear(c);
  }

  // register r of a lane's tile is feature 4 q + r, column i of the tile
  const int cells = a.D * MP;
  float* const out = a.part + ((int64_t)blockIdx.y * W + blockIdx.x) * cells;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = (wf * RT + rt) * 16 + 4 * q + r;
      if (f >= a.D) continue;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) out[f * MP + (wc * CT + ct) * 16 + i] = acc[rt][ct][r];
      if (with_sum && i == 0) a.psum[(int64_t)blockIdx.x * a.D + f] = sum[rt][r];
    }
}

// dT[j, col] and dsum[j] = the work-groups' partials, added in ascending order of the work-group.
// One thread per element of dT, then one per element of dsum.
__global__ __launch_bounds__(256) void weight_grad16_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ psum, int32_t groups, int32_t mp,
    float* __restrict__ dT, int64_t dts, float* __restrict__ dsum, int32_t D, int32_t M) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t cells = (int64_t)D * M;
  if (e < cells) {
    const int j = (int)(e / M), col = (int)(e % M);
    const int64_t slab = (int64_t)D * mp;
    const float* p = part + (int64_t)(col / mp) * groups * slab + (int64_t)j * mp + col % mp;
    float v = 0.f;
    for (int32_t w = 0; w < groups; ++w) v = v + p[w * slab];
    dT[j * dts + col] = v;
  } else if (dsum && e < cells + D) {
    const int j = (int)(e - cells);
    float v = 0.f;
    for (int32_t w = 0; w < groups; ++w) v = v + psum[(int64_t)w * D + j];
    dsum[j] = v;
  }
}

// a [rows, width] array of `stride` elements per row: the bytes from its first to its last element
static int64_t span(int64_t rows, int64_t stride, int64_t width, int64_t elem) {
  return rows > 0 ? elem * ((rows - 1) * stride + width) : 0;
}

static int weight_grad16(const float* data, int64_t ds, const uint8_t* sel, int64_t is,
                         const void* g, int64_t gs, int32_t dtype, float* dT, int64_t dts,
                         float* dsum, void* scratch, int64_t sbytes, int32_t N, int32_t D,
                         int32_t k, int32_t M, void* stream) {
  const std::string w("maxk_cbsr_weight_grad_16: ");
  MAXK_CHECK_ARG(dtype == MAXK_DTYPE_BF16 || dtype == MAXK_DTYPE_F16,
                 w + "dtype must be MAXK_DTYPE_BF16 or MAXK_DTYPE_F16");
  MAXK_CHECK_ARG(N >= 0 && M >= 1, w + "num_rows must be >= 0 and dim_m >= 1");
  if (D > maxk::kMaxDim) {
    set_error(w + "dim_origin above 256 is not supported (u8 selectors)");
    return MAXK_ERR_UNSUPPORTED;
  }
  MAXK_CHECK_ARG(k >= 1 && k <= D, w + "k must be between 1 and input dimension");
  const int64_t P = panel_count(M);
  if (P > kMaxPanels) {
    set_error(w + "dim_m beyond the grid's 65535 panels is not supported");
    return MAXK_ERR_UNSUPPORTED;
  }
  if (ds == 0) ds = k;
  if (is == 0) is = k;
  if (gs == 0) gs = M;
  if (dts == 0) dts = M;
  MAXK_CHECK_ARG(ds >= k, w + "data_stride must be >= k (0: k)");
  MAXK_CHECK_ARG(is >= k, w + "index_stride must be >= k (0: k)");
  MAXK_CHECK_ARG(gs >= M, w + "g_stride must be >= dim_m (0: dim_m)");
  MAXK_CHECK_ARG(dts >= M, w + "grad_table_stride must be >= dim_m (0: dim_m)");
  const int64_t need = scratch_bytes(N, D, k, M);
  MAXK_CHECK_ARG(sbytes >= need,
                 w + "scratch_bytes is below maxk_cbsr_weight_grad_16_scratch_bytes");
  MAXK_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 15) == 0,
                 w + "scratch must be 16-B aligned");
  const Range ins[3] = {{data, span(N, ds, k, 4)}, {sel, span(N, is, k, 1)},
                        {g, span(N, gs, M, 2)}};
  const Range outs[3] = {{dT, span(D, dts, M, 4)}, {dsum, dsum ? 4 * (int64_t)D : 0},
                         {scratch, need}};
  if (int rc = check_ranges(w, ins, 3, outs, 3)) return rc;
  const int32_t W = row_groups(N, P);
  const int mp = panel_width(M);
  float* part = (float*)scratch;
  float* psum = part + P * W * D * mp;
  if (N > 0) {
    const Args a{data, ds, sel, is, static_cast<const uint16_t*>(g), gs, part,
                 dsum ? psum : nullptr, N, D, k, M};
    if (int e = maxk::dispatch_variant(
            kWeightGrad16Variants, select_weight_grad16_variant(D, M, dtype),
            [&](auto idx) -> int {
              constexpr WeightGrad16Variant V = kWeightGrad16Variants[decltype(idx)::value];
              hipLaunchKernelGGL((weight_grad16_kernel<V.dp, V.mp, V.dtype>),
                                 dim3((unsigned)W, (unsigned)P), dim3(kThreads), 0,
                                 (hipStream_t)stream, a);
              return MAXK_OK;
            }))
      return e;
  }
  const int64_t threads = (int64_t)D * M + D;
  hipLaunchKernelGGL(weight_grad16_reduce_kernel, dim3((unsigned)((threads + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, (const float*)part, (const float*)psum,
                     N > 0 ? W : 0, mp, dT, dts, dsum, D, M);
  MAXK_LAUNCH_CHECK("maxk_cbsr_weight_grad_16 launch");
  return MAXK_OK;
}

}  // namespace maxk_wg16

extern "C" int maxk_cbsr_weight_grad_16(const float* sp_data, int64_t data_stride,
                                        const uint8_t* sp_index, int64_t index_stride,
                                        const void* g, int64_t g_stride, int32_t dtype,
                                        float* grad_table, int64_t grad_table_stride,
                                        float* grad_sum, void* scratch, int64_t scratch_bytes,
                                        int32_t num_rows, int32_t dim_origin, int32_t dim_k,
                                        int32_t dim_m, void* stream) {
  return maxk_wg16::weight_grad16(sp_data, data_stride, sp_index, index_stride, g, g_stride, dtype,
                                  grad_table, grad_table_stride, grad_sum, scratch, scratch_bytes,
                                  num_rows, dim_origin, dim_k, dim_m, stream);
}

extern "C" int64_t maxk_cbsr_weight_grad_16_scratch_bytes(int32_t num_rows, int32_t dim_origin,
                                                          int32_t dim_k, int32_t dim_m) {
  return maxk_wg16::scratch_bytes(num_rows, dim_origin, dim_k, dim_m);
}

extern "C" int maxk_cbsr_weight_grad_16_tile(int32_t dim_origin, int32_t dim_m, int32_t* out,
                                             int32_t capacity) {
  if (dim_origin < 1 || dim_origin > maxk::kMaxDim || dim_m < 1) return 0;
  const int64_t panels = maxk_wg16::panel_count(dim_m);
  const int dp = maxk_wg16::padded_dim(dim_origin), mp = maxk_wg16::panel_width(dim_m);
  return maxk::copy_limits(out, capacity,
                           {dp, mp, (int32_t)(panels < INT32_MAX ? panels : INT32_MAX),
                            maxk_wg16::kChunkRows, maxk_wg16::group_cap(panels),
                            maxk_wg16::lds_bytes(dp, mp)});
}
