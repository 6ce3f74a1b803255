// CBSR rows times a 16-bit table on the matrix cores (include/maxk_hip.h, "MaxK linear layers,
// 16-bit CBSR product"): with the CBSR tables v [N, k] f32 and s [N, k] u8 and a bf16 or f16 table
// T [D, M],
//
//   vr        = v rounded to the type of T
//   out[n, :] = sum_l vr[n, l] T[s[n, l], :]
//
// as the dense-shaped product densify(vr) [N, D] @ T [D, M] on v_mfma_f32_16x16x32_bf16 / _f16. It
// is the input gradient of the 16-bit fused linear + MaxK. The densified rows are mostly zeros,
// which costs arithmetic that these instructions have to spare, and buys a kernel without a
// per-slot LDS gather whose summation order is fixed. The densified rows are never in memory: they
// are built, 128 rows at a time, in LDS.
//
// Work split. A work-group of 8 waves owns one panel of MP = 128 or 64 columns of M (blockIdx.y) and
// a contiguous range of 128-row tiles (blockIdx.x); all panels together are at most kGroups
// work-groups. It stages T[:, panel] in LDS once, [DP][MP + 16] with DP = D rounded up to 64, 128
// or 256 (rows past D and columns past M are zeros), and keeps it there. Wave w owns rows
// 16 w .. 16 w + 15 of every tile from the first load to the last store: its threads fetch those
// rows' slots, build their densified rows, multiply them with the whole panel (MP / 16 accumulator
// tiles of 16 x 16, 32 registers a lane at MP = 128) and store their [16, MP] of out. No wave reads
// what another wave wrote after the panel is staged, so the tile loop has no barrier in it: the
// one __syncthreads behind the staging orders the panel's stores (and the clearing of the densified
// tile) against the other waves' reads, and inside a wave the LDS operations keep their order.
//
// Data movement, per tile:
//   * 4 threads share a row's slots (slot l0 + 4 j, 16 of them held in registers: k <= 64; slots
//     past 64 are read again when they are used). They are loaded, the values rounded and packed,
//     while the matrix cores work on the tile before.
//   * The densified tile [128][DP + 8] lives in LDS, zeroed once. A slot writes its rounded value at
//     [row][position of its selector] with one 2-byte store, and after the tile's MFMAs the same
//     thread writes zero there again. A selector >= D stores nowhere. The 32 features of a depth
//     step are permuted over its positions (depth_position, variants_matmul16.h) so that lane
//     (i, q) reads its 8 positions of row i with one ds_read_b128 while the two transposing reads of
//     the panel take features 4 q ... and 16 + 4 q ..., 16 different panel rows a read.
//   * The panel's operand is 8 features of one column: ds_read_b64_tr_b16 delivers four of them a
//     read from the row-major panel (in a group of 16 lanes, lane l reads the 8 bytes at row l / 4,
//     elements 4 (l % 4) ...; lane i receives element i of those four rows).
//   * The panel is the MFMA's first operand and the densified rows its second, so register r of lane
//     (i, q) is row i, staged column 16 t + 4 q + r of tile t. The columns of a 32-column group are
//     staged permuted (staged_column) so that those of tiles 2 c and 2 c + 1 are the 8 consecutive
//     columns 32 c + 8 q ...: one 16-byte store of a 16-bit row, two of an f32 row, where base and
//     stride allow; guarded single stores otherwise.
//
// No plan, no scratch, no atomics, nothing allocated, capturable; every array takes a row stride.
#include "common.h"
#include "variants_matmul16.h"

namespace maxk_mm16 {

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
  const uint16_t* T;  // bits of bf16 or f16
  int64_t ts;
  void* out;          // f32, or bits of the type
  int64_t os;
  int32_t out16;      // the output is of the type
  int32_t N, D, k, M;
};

template <class K>
static hipError_t allow_lds(K* kernel, size_t bytes) {
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)bytes);
}

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

// ds_read_b64_tr_b16 at p (LDS, 8-byte aligned): four rows of this lane's element
__device__ __forceinline__ uint2 read_transposed(const uint16_t* p) {
  typedef __attribute__((address_space(3))) i16x4 lds_i16x4;
  return __builtin_bit_cast(
      uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)const_cast<uint16_t*>(p)));
}

// The wave's LDS stores before, its LDS reads behind (or the other way round): the hardware keeps a
// wave's LDS operations in order, this keeps the compiler from changing it
__device__ __forceinline__ void wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Position of feature s in a densified row
__device__ __forceinline__ int feature_position(int s) {
  return (s & ~(kStep - 1)) | depth_position(s & (kStep - 1));
}

template <int DP, int MP, int kDtype>
__global__ __launch_bounds__(kThreads)
__attribute__((amdgpu_waves_per_eu(waves_per_simd(DP, MP), waves_per_simd(DP, MP))))
void matmul16_kernel(const Args a) {
  constexpr int CT = MP / 16;       // accumulator tiles of a wave: all columns of the panel
  constexpr int TS = MP + kTPad;    // elements of a staged row of the panel
  constexpr int AR = DP + kAPad;    // elements of a densified row
  constexpr int LPR = MP / 8;       // 16-byte loads a row of the panel
  static_assert(kThreads == kTileRows * kSlotLanes && kWave == kWaveRows * kSlotLanes &&
                (2 * TS) % 16 == 0 && (2 * AR) % 16 == 0 && CT % 2 == 0 && DP % kStep == 0,
                "tile walk below");
  extern __shared__ __align__(16) uint16_t smem[];
  uint16_t* const tl = smem;            // T[:, panel], [DP][TS], columns staged permuted
  uint16_t* const at = smem + DP * TS;  // densified rows [128][AR]

  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int i = lane & 15, q = lane >> 4;
  const int p0 = blockIdx.y * MP, W = gridDim.x;
  const int64_t tiles = ((int64_t)a.N + kTileRows - 1) / kTileRows;
  const int64_t t_begin = tiles * blockIdx.x / W, t_end = tiles * (blockIdx.x + 1) / W;

  // this thread's part of the slot pass: row srow of the tile (one of its wave's), slots sl, sl + 4, ...
  const int srow = tid / kSlotLanes, sl = tid % kSlotLanes;
  uint16_t* const at_mine = at + srow * AR;

  // the first 16 slots of the thread: rounded values two a register, selectors four a register, one
  // bit a slot that is there (not past k, not of a row past N, selector below D)
  uint32_t pre_v[kSlotsHeld / 2], pre_s[kSlotsHeld / 4], cur_s[kSlotsHeld / 4];
  uint32_t pre_on = 0, cur_on = 0;
  auto load = [&](int64_t t) {
    const int64_t row = t * kTileRows + srow;
    pre_on = 0;
#pragma unroll
    for (int j = 0; j < kSlotsHeld; ++j) {
      const int l = sl + kSlotLanes * j;
      bool on = row < a.N && l < a.k;
      const uint32_t s = on ? a.sel[row * a.is + l] : 0u;
      on = on && s < (uint32_t)a.D;
      const uint32_t v = on ? round16<kDtype>(a.data[row * a.ds + l]) : 0u;
      pre_v[j / 2] = j % 2 ? pre_v[j / 2] | v << 16 : v;
      pre_s[j / 4] = j % 4 ? pre_s[j / 4] | s << 8 * (j % 4) : s;
      pre_on |= (on ? 1u : 0u) << j;
    }
  };
  // the tile's values into the wave's densified rows
  auto stage = [&](int64_t t) {
    cur_on = pre_on;
#pragma unroll
    for (int j = 0; j < kSlotsHeld; ++j) {
      cur_s[j / 4] = pre_s[j / 4];
      if (pre_on >> j & 1u)
        at_mine[feature_position(pre_s[j / 4] >> 8 * (j % 4) & 0xffu)] =
            (uint16_t)(pre_v[j / 2] >> 16 * (j % 2));
    }
    const int64_t row = t * kTileRows + srow;
    if (row >= a.N) return;
    for (int l = sl + kSlotLanes * kSlotsHeld; l < a.k; l += kSlotLanes) {  // k > 64
      const int s = a.sel[row * a.is + l];
      if (s < a.D) at_mine[feature_position(s)] = (uint16_t)round16<kDtype>(a.data[row * a.ds + l]);
    }
  };
  // zeros again where the tile's slots wrote, behind its MFMAs
  auto clear = [&](int64_t t) {
#pragma unroll
    for (int j = 0; j < kSlotsHeld; ++j)
      if (cur_on >> j & 1u) at_mine[feature_position(cur_s[j / 4] >> 8 * (j % 4) & 0xffu)] = 0;
    const int64_t row = t * kTileRows + srow;
    if (row >= a.N) return;
    for (int l = sl + kSlotLanes * kSlotsHeld; l < a.k; l += kSlotLanes) {
      const int s = a.sel[row * a.is + l];
      if (s < a.D) at_mine[feature_position(s)] = 0;
    }
  };

  if (t_begin < t_end) load(t_begin);
  // the panel, once: 8 columns a load, the two halves of which go to the two tiles of their group
  {
    const bool vec = ((reinterpret_cast<uintptr_t>(a.T) & 15) | (uintptr_t)(a.ts & 7)) == 0;
    for (int e = tid; e < DP * LPR; e += kThreads) {
      const int row = e / LPR, col = 8 * (e % LPR);
      const bool on = row < a.D;
      const uint4 v = load_chunk8(a.T + (on ? row : 0) * a.ts, p0 + col, a.M, on, vec);
      uint16_t* const dst = tl + row * TS + (col & ~31) + staged_column(col & 31);
      *reinterpret_cast<uint2*>(dst) = make_uint2(v.x, v.y);
      *reinterpret_cast<uint2*>(dst + 16) = make_uint2(v.z, v.w);
    }
    for (int e = tid; e < kTileRows * AR / 8; e += kThreads)
      reinterpret_cast<uint4*>(at)[e] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();  // the panel is staged and the densified tile is zeros: the only barrier

  const uint16_t* const ar = at + (wave * kWaveRows + i) * AR + 8 * q;
  const uint16_t* const br = tl + (4 * q + (i >> 2)) * TS + 4 * (i & 3);
  const int esize = a.out16 ? 2 : 4;
  const bool wide = ((reinterpret_cast<uintptr_t>(a.out) & 15) | (uintptr_t)(a.os * esize & 15)) == 0;

  for (int64_t t = t_begin; t < t_end; ++t) {
    stage(t);
    wave_order();  // the wave's stores, then its reads
    if (t + 1 < t_end) load(t + 1);  // uniform
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < DP; kb += kStep) {
      const uint4 av = *reinterpret_cast<const uint4*>(ar + kb);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const uint2 lo = read_transposed(br + kb * TS + ct * 16);               // features 4 q ...
        const uint2 hi = read_transposed(br + (kb + kStep / 2) * TS + ct * 16);  // 16 + 4 q ...
        acc[ct] = mfma_step<kDtype>(make_uint4(lo.x, lo.y, hi.x, hi.y), av, acc[ct]);
      }
    }
    wave_order();  // the wave's reads, then its zeros
    clear(t);

    // registers of tiles 2 c and 2 c + 1 of lane (i, q): row i, columns 32 c + 8 q + 0 .. 7
    const int64_t row = t * kTileRows + wave * kWaveRows + i;
    if (row >= a.N) continue;
#pragma unroll
    for (int c = 0; c < CT / 2; ++c) {
      const int col = p0 + 32 * c + 8 * q;
      if (col >= a.M) continue;
      const f32x4 x = acc[2 * c], y = acc[2 * c + 1];
      const bool whole = wide && col + 7 < a.M;
      if (a.out16) {
        uint16_t* const o = static_cast<uint16_t*>(a.out) + row * a.os + col;
        uint32_t b[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          b[r] = round16<kDtype>(x[r]);
          b[4 + r] = round16<kDtype>(y[r]);
        }
        if (whole) {
          *reinterpret_cast<uint4*>(o) = make_uint4(b[0] | b[1] << 16, b[2] | b[3] << 16,
                                                    b[4] | b[5] << 16, b[6] | b[7] << 16);
        } else {
#pragma unroll
          for (int r = 0; r < 8; ++r)
            if (col + r < a.M) o[r] = (uint16_t)b[r];
        }
      } else {
        float* const o = static_cast<float*>(a.out) + row * a.os + col;
        if (whole) {
          *reinterpret_cast<f32x4*>(o) = x;
          *reinterpret_cast<f32x4*>(o + 4) = y;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (col + r < a.M) o[r] = x[r];
            if (col + 4 + r < a.M) o[4 + r] = y[r];
          }
        }
      }
    }
  }
}

// a [rows, width] array of `stride` elements per row: the bytes from its first to its last element
static int64_t span(int64_t rows, int64_t stride, int64_t width, int64_t elem) {
  return rows > 0 ? elem * ((rows - 1) * stride + width) : 0;
}

static int matmul16(const float* data, int64_t ds, const uint8_t* sel, int64_t is, const void* T,
                    int64_t ts, int32_t dtype, void* out, int64_t os, int32_t out_dtype, int32_t N,
                    int32_t D, int32_t k, int32_t M, void* stream) {
  const std::string w("maxk_cbsr_matmul_16: ");
  MAXK_CHECK_ARG(dtype == MAXK_DTYPE_BF16 || dtype == MAXK_DTYPE_F16,
                 w + "dtype must be MAXK_DTYPE_BF16 or MAXK_DTYPE_F16");
  MAXK_CHECK_ARG(out_dtype == 0 || out_dtype == dtype, w + "out_dtype must be 0 (f32) or dtype");
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
  if (ts == 0) ts = M;
  if (os == 0) os = M;
  MAXK_CHECK_ARG(ds >= k, w + "data_stride must be >= k (0: k)");
  MAXK_CHECK_ARG(is >= k, w + "index_stride must be >= k (0: k)");
  MAXK_CHECK_ARG(ts >= M, w + "table_stride must be >= dim_m (0: dim_m)");
  MAXK_CHECK_ARG(os >= M, w + "out_stride must be >= dim_m (0: dim_m)");
  const Range ins[3] = {{data, span(N, ds, k, 4)}, {sel, span(N, is, k, 1)},
                        {T, span(D, ts, M, 2)}};
  const Range outs[1] = {{out, span(N, os, M, out_dtype ? 2 : 4)}};
  if (int rc = check_ranges(w, ins, 3, outs, 1)) return rc;
  if (N == 0) return MAXK_OK;
  const Args a{data, ds, sel, is, static_cast<const uint16_t*>(T), ts, out, os,
               out_dtype != 0, N, D, k, M};
  if (int e = maxk::dispatch_variant(
          kMatmul16Variants, select_matmul16_variant(D, M, dtype), [&](auto idx) -> int {
            constexpr Matmul16Variant V = kMatmul16Variants[decltype(idx)::value];
            auto kern = matmul16_kernel<V.dp, V.mp, V.dtype>;
            constexpr size_t lds = lds_bytes(V.dp, V.mp);
            if (lds > 64 * 1024) MAXK_HIP_TRY(allow_lds(kern, lds));
            hipLaunchKernelGGL(kern, dim3((unsigned)row_groups(N, P), (unsigned)P),
                               dim3(kThreads), lds, (hipStream_t)stream, a);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_cbsr_matmul_16 launch");
  return MAXK_OK;
}

}  // namespace maxk_mm16

extern "C" int maxk_cbsr_matmul_16(const float* sp_data, int64_t data_stride,
                                   const uint8_t* sp_index, int64_t index_stride,
                                   const void* table, int64_t table_stride, int32_t dtype,
                                   void* out, int64_t out_stride, int32_t out_dtype,
                                   int32_t num_rows, int32_t dim_origin, int32_t dim_k,
                                   int32_t dim_m, void* stream) {
  return maxk_mm16::matmul16(sp_data, data_stride, sp_index, index_stride, table, table_stride,
                             dtype, out, out_stride, out_dtype, num_rows, dim_origin, dim_k, dim_m,
                             stream);
}

extern "C" int maxk_cbsr_matmul_16_tile(int32_t dim_origin, int32_t dim_m, int32_t* out,
                                        int32_t capacity) {
  if (dim_origin < 1 || dim_origin > maxk::kMaxDim || dim_m < 1) return 0;
  const int64_t panels = maxk_mm16::panel_count(dim_m);
  const int dp = maxk_mm16::padded_dim(dim_origin), mp = maxk_mm16::panel_width(dim_m);
  return maxk::copy_limits(out, capacity,
                           {dp, mp, (int32_t)(panels < INT32_MAX ? panels : INT32_MAX),
                            maxk_mm16::kTileRows, maxk_mm16::group_cap(panels),
                            maxk_mm16::lds_bytes(dp, mp)});
}
