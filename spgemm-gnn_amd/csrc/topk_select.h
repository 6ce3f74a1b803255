// The per-row top-k of a wave that holds a row as four consecutive features per lane: the order key,
// the wave-wide DPP scans, the exact radix selection and the emission of the selected entries
// (tables, records, dense masked row, dropout, statistics). Shared by the top-k kernels
// (maxk_topk.hip) and the fused linear + top-k kernel (linear_topk.hip); device code only.
#pragma once

#include "common.h"

namespace maxk {

constexpr int kTopkThreads = 256;  // 4 rows (waves) per work-group

__device__ __forceinline__ uint32_t order_key(float x) {
  // Monotone map f32 -> u32: larger float => larger key (+0 > -0). Every NaN, of either sign
  // and any payload, maps to the largest key, so NaNs rank above +Inf and tie with each other
  // (ties to the lowest feature index): torch.topk's order (its radix key sends NaN to
  // 0xffffffff), which the reference trains with (utils/models.py:15).
  const uint32_t b = __float_as_uint(x);
  const uint32_t key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (b & 0x7fffffffu) > 0x7f800000u ? 0xffffffffu : key;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
  // popcount(mask & ((1 << lane) - 1))
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

// Feature dropout fused into the top-k and the scatter (maxk_hip.h, "Dropout mask"): a
// counter-based keep bit per (seed, global row, feature), no mask tensor. DropArg<false> is
// empty, so the kernels without dropout carry nothing of it.
template <bool kDrop>
struct DropArg {};
template <>
struct DropArg<true> {
  uint32_t lo, hi;   // the 64-bit seed
  uint32_t thresh;   // T: an entry is kept when its draw u >= T
  uint32_t row_lo;   // low word of row_offset
  float scale;       // 1 / (1 - p); 0 when p == 1: nothing is kept, whatever u
};

__device__ __forceinline__ uint32_t fmix32(uint32_t x) {  // murmur3 finaliser
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

// The two per-row words of the mask, wave-uniform (scalar registers): `row` must be the same
// in every lane of the wave.
struct DropRow {
  uint32_t a, b;
  __device__ __forceinline__ DropRow(const DropArg<true>& d, int row) {
    const uint32_t R = __builtin_amdgcn_readfirstlane((uint32_t)row + d.row_lo);
    a = fmix32(R ^ d.lo);
    b = fmix32(R * 0x9E3779B1u + d.hi);
  }
  // x after dropout at feature f: scaled when kept, +0.0f when dropped (also for Inf / NaN)
  __device__ __forceinline__ float apply(const DropArg<true>& d, uint32_t f, float x) const {
    const uint32_t u = fmix32(fmix32(a + 0x9E3779B1u * (f + 1u)) ^ b);
    return (d.scale != 0.f && u >= d.thresh) ? __fmul_rn(x, d.scale) : 0.f;
  }
};

// Dense masked row of maxk_topk_cbsr_dense: row r at p + r * stride (floats). DenseArg<false> is
// empty, as DropArg<false>.
template <bool kDense>
struct DenseArg {};
template <>
struct DenseArg<true> {
  float* p;
  int64_t stride;
};

// Inclusive prefix sum over the 64 lanes with DPP (no LDS round trips): row_shr 1/2/4/8
// within each 16-lane row, then row_bcast:15 / row_bcast:31 across rows (GFX9 family).
__device__ __forceinline__ uint32_t wave_prefix_sum(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);  // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return (uint32_t)x;
}

// Wave-wide reductions as DPP inclusive scans (same shifts as wave_prefix_sum) read from
// lane 63: VALU-only, where __shfl_xor is a chain of 6 dependent ds_bpermute round trips.
// Lanes without a source take `id`, the operation's identity.
template <class Op>
__device__ __forceinline__ uint32_t wave_reduce_dpp(uint32_t v, uint32_t id, Op op) {
  int x = (int)v;
  x = (int)op((uint32_t)x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, x, 0x111, 0xf, 0xf, false));
  x = (int)op((uint32_t)x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, x, 0x112, 0xf, 0xf, false));
  x = (int)op((uint32_t)x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, x, 0x114, 0xf, 0xf, false));
  x = (int)op((uint32_t)x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, x, 0x118, 0xf, 0xf, false));
  x = (int)op((uint32_t)x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, x, 0x142, 0xa, 0xf, false));
  x = (int)op((uint32_t)x, (uint32_t)__builtin_amdgcn_update_dpp((int)id, x, 0x143, 0xc, 0xf, false));
  return (uint32_t)__builtin_amdgcn_readlane(x, kWave - 1);
}

__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
  return wave_reduce_dpp(v, 0u, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
}

__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
  return wave_reduce_dpp(v, 0xffffffffu, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
}

// Fixed-point statistics of the emitted rows (the pair maxk_cbsr_stats computes over the table,
// spgemm.hip cbsr_stats4_kernel): per lane, the largest and the smallest nonzero |x| bit pattern
// among the entries it emits. Emitted rows never repeat a selector and store them ascending, so
// a row's slot bound is its max |x| (no row sum needed).
struct TopkStats {
  uint32_t mx = 0u, mn = 0x7fffffffu;
  __device__ __forceinline__ void add(float x) {
    const uint32_t b = __float_as_uint(x) & 0x7fffffffu;
    if (b != 0u) {
      mx = max(mx, b);
      mn = min(mn, b);
    }
  }
  // Wave reduction, then one work-group pair through LDS (`red`: 2 words per wave), stored by
  // thread 0 as this work-group's partial pair (plain stores: same-address atomics from every
  // work-group serialise at the memory side and cost the top-k ~35 us at Reddit, round 6);
  // topk_stats_reduce_kernel combines the partials. Every wave of the work-group must call this.
  // Wave reduction only, stored by lane 0 as partial pair `slot` (no barrier: the exact kernel's
  // waves retire on their own). Slot 0 also zeroes the launch's result pair.
  __device__ __forceinline__ void flush_wave(uint32_t* part, int64_t slot, uint32_t* pair) {
    const uint32_t wm = wave_umax(mx), wn = wave_umin(mn);
    if ((threadIdx.x & (kWave - 1)) == 0) {
      part[2 * slot] = wm;
      part[2 * slot + 1] = 0x7fffffffu - wn;
      if (slot == 0) {  // the reduce launch that follows adds into it
        pair[0] = 0u;
        pair[1] = 0u;
      }
    }
  }
  template <int kWaves>
  __device__ __forceinline__ void flush(uint32_t* red, uint32_t* part, uint32_t* pair) {
    const uint32_t wm = wave_umax(mx), wn = wave_umin(mn);
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (lane == 0) {
      red[2 * w] = wm;
      red[2 * w + 1] = wn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t a = red[0], b = red[1];
#pragma unroll
      for (int i = 1; i < kWaves; ++i) {
        a = max(a, red[2 * i]);
        b = min(b, red[2 * i + 1]);
      }
      part[2 * blockIdx.x] = a;
      part[2 * blockIdx.x + 1] = 0x7fffffffu - b;
      if (blockIdx.x == 0) {  // the reduce launch that follows adds into it
        pair[0] = 0u;
        pair[1] = 0u;
      }
    }
  }
};

__device__ __forceinline__ float wave_min(float v) {
  return __uint_as_float(wave_reduce_dpp(__float_as_uint(v), __float_as_uint(__builtin_inff()),
                                         [](uint32_t a, uint32_t b) {
                                           return __float_as_uint(fminf(__uint_as_float(a), __uint_as_float(b)));
                                         }));
}
__device__ __forceinline__ float wave_max(float v) {
  return __uint_as_float(wave_reduce_dpp(__float_as_uint(v), __float_as_uint(-__builtin_inff()),
                                         [](uint32_t a, uint32_t b) {
                                           return __float_as_uint(fmaxf(__uint_as_float(a), __uint_as_float(b)));
                                         }));
}

// Loads the 4 features [4*lane, 4*lane+4) of row `row` (guarded by D).
__device__ __forceinline__ void load_row4(const float* __restrict__ in, int row, int D,
                                          int lane, float x[4], bool valid[4]) {
  const int j0 = lane * 4;
  const float* src = in + (size_t)row * D;
  if ((D & 3) == 0 && j0 < D) {
    float4 v = *reinterpret_cast<const float4*>(src + j0);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
#pragma unroll
    for (int i = 0; i < 4; ++i) valid[i] = true;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      valid[i] = (j0 + i) < D;
      x[i] = valid[i] ? src[j0 + i] : 0.f;
    }
  }
}

// Record destination of maxk_topk_cbsr_records: row r's forward record (maxk_plan_info.fwd_layout
// 1, 2 or 4) starts at p + r * bytes.
struct TopkRec {
  uint8_t* p = nullptr;
  int bytes = 0;
  int layout = 0;
};

// One row's forward record from the wave's staging rows (the k entries in output order), as the
// forward's own pack passes write it (spgemm.hip: cbsr_stats4_kernel PACK 1 / 2,
// pack_cbsr3_kernel): lane j stores chunk j with one 16-B store (at most 64 chunks, so one store
// per lane also covers k > 64); bytes past the last chunk stay unwritten.
//   4: pair chunk  {x[2j], x[2j+1], sel[2j] | sel[2j+1] << 8, 0}                  (k even)
//   2: lane chunk  {x[3j], x[3j+1], x[3j+2], sel[3j] | sel[3j+1] << 8 | sel[3j+2] << 16},
//      slots >= k zero
//   1: k values at byte 0, k selector bytes at byte 4k                            (k % 4 == 0)
__device__ __forceinline__ void store_record(const float* stage_v, const uint8_t* stage_i,
                                             int lane, int k, uint8_t* rp, int layout) {
  if (layout == 4) {
    if (lane < k / 2) {
      const float2 v = reinterpret_cast<const float2*>(stage_v)[lane];
      const uint32_t s = reinterpret_cast<const uint16_t*>(stage_i)[lane];
      reinterpret_cast<uint4*>(rp)[lane] =
          make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), s, 0u);
    }
  } else if (layout == 2) {
    if (lane < (k + 2) / 3) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int l = 3 * lane + i;
        if (l < k) {
          w[i] = __float_as_uint(stage_v[l]);
          w[3] |= (uint32_t)stage_i[l] << (8 * i);
        }
      }
      reinterpret_cast<uint4*>(rp)[lane] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  } else {
    for (int j = lane; j < k; j += kWave) reinterpret_cast<float*>(rp)[j] = stage_v[j];
    if (lane < k / 4)
      reinterpret_cast<uint32_t*>(rp + 4 * k)[lane] = reinterpret_cast<const uint32_t*>(stage_i)[lane];
  }
}

// Writes the selected entries in ascending feature order: position of (lane,i) =
// number of selected entries with a smaller feature index.
__device__ __forceinline__ int emit_selected(const float x[4], const bool sel[4], int lane,
                                             int row, int k, float* __restrict__ sp_data,
                                             uint8_t* __restrict__ sp_index, int ds, int is,
                                             TopkStats* st = nullptr) {
  uint64_t m[4];
  int total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m[i] = __ballot(sel[i]);
    total += __popcll(m[i]);
  }
  int pos = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) pos += (int)lanes_below(m[i]);
  float* drow = sp_data + (size_t)row * ds;
  uint8_t* irow = sp_index + (size_t)row * is;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (sel[i]) {
      if (pos < k) {
        drow[pos] = x[i];
        irow[pos] = (uint8_t)(lane * 4 + i);
        if (st) st->add(x[i]);
      }
      ++pos;
    }
  }
  return total;
}

// emit_selected through the wave's LDS staging rows: the selected entries are written to
// stage_v/stage_i at their output position, then each output row leaves in coalesced stores
// (dwords of values, dwords of four selectors) instead of 2x4 scattered per-lane stores
// (exact top-k: Reddit k=16 0.069 -> 0.067 ms, ogbn-products 0.688 -> 0.647 ms with 8 rows per
// wave, profiles/r03/topk_probe.jsonl).
// kWide: k > 64 (the store loops cost the k <= 64 kernels 11 VGPRs, so they get their own).
// kRec (maxk_topk_cbsr_records): the row's forward record is stored from the same staging rows
// (store_record), and either plain table may be absent (null).
// kDrop (maxk_topk_cbsr_dropout, with kRec): the dropout mask is applied to the staged values
// in place, by the lane that then stores slot j (one draw per slot: masking the four candidates
// of every lane as they enter the staging rows cost 4 draws per lane and row, +23 us on the
// 84 us Reddit k = 16 top-k), before anything leaves the staging rows, so tables, record and
// statistics all see the dropped, scaled values; the record may be absent too (rec.p null).
// kDense (maxk_topk_cbsr_dense, with kRec): the dense masked row too, one float4 per lane from
// the registers that hold the row: x[i] where (lane, i) fills a slot, +0.0f elsewhere (also for
// a ref_compat entry with x > p past slot k). With kDrop the lane remembers its first slot,
// walks its staged features again and reads each dropped, scaled value back from the staging
// row after the fence that follows the draw, so the mask is still drawn once per slot. Tables and record are
// all optional. D: the row's features (partial rows store scalars).
template <bool kWide, bool kRec = false, bool kDrop = false, bool kDense = false>
__device__ __forceinline__ void emit_staged(const float x[4], const bool sel[4], int lane, int row,
                                            int k, float* stage_v, uint8_t* stage_i,
                                            float* __restrict__ sp_data,
                                            uint8_t* __restrict__ sp_index, int ds, int is,
                                            TopkStats* st = nullptr, TopkRec rec = TopkRec{},
                                            const DropArg<kDrop>& drop = DropArg<kDrop>{},
                                            const DenseArg<kDense>& dense = DenseArg<kDense>{},
                                            int D = 4 * kWave) {
  static_assert(kRec || !kDense, "the dense variant takes every table as optional");
  uint64_t m[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = __ballot(sel[i]);
  int pos = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) pos += (int)lanes_below(m[i]);
  [[maybe_unused]] const int pos0 = pos;  // kDense: the slot of this lane's first entry
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (sel[i]) {
      if (pos < k) {
        stage_v[pos] = x[i];
        stage_i[pos] = (uint8_t)(lane * 4 + i);
      }
      ++pos;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float* drow = sp_data + (size_t)row * ds;
  uint8_t* irow = sp_index + (size_t)row * is;
  const bool put_v = !kRec || sp_data != nullptr;   // wave-uniform
  const bool put_i = !kRec || sp_index != nullptr;
  [[maybe_unused]] const auto drop_row = [&] {  // the row's two mask words, once per row
    if constexpr (kDrop) return DropRow(drop, row); else return 0;
  }();
  if constexpr (!kWide) {
    if (lane < k) {
      float v = stage_v[lane];
      if constexpr (kDrop) {  // slot `lane` is this lane's alone until the fence below
        v = drop_row.apply(drop, stage_i[lane], v);
        stage_v[lane] = v;
      }
      if (put_v) drow[lane] = v;
      if (st) st->add(v);  // statistics of the stored entry (one per lane and row)
    }
    if (put_i && ((k | is) & 3) == 0) {  // row * is a multiple of 4: dword-aligned selector rows
      if (lane < k / 4)
        reinterpret_cast<uint32_t*>(irow)[lane] = reinterpret_cast<const uint32_t*>(stage_i)[lane];
    } else if (put_i && lane < k) {
      irow[lane] = stage_i[lane];
    }
  } else {
    for (int j = lane; j < k; j += kWave) {
      float v = stage_v[j];
      if constexpr (kDrop) {
        v = drop_row.apply(drop, stage_i[j], v);
        stage_v[j] = v;
      }
      if (put_v) drow[j] = v;
      if (put_i) irow[j] = stage_i[j];
      if (st) st->add(v);
    }
  }
  if constexpr (kRec) {
    if constexpr (kDrop) {  // the record's lanes read slots other lanes have just rewritten
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if ((!kDrop && !kDense) || rec.p != nullptr)  // wave-uniform
      store_record(stage_v, stage_i, lane, k, rec.p + (size_t)row * rec.bytes, rec.layout);
  }
  if constexpr (kDense) {
    // the lane's slots again, from its first one and the ballots (scalar registers)
    float o[4];
    int q = pos0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = 0.f;
      if ((m[i] >> lane) & 1) {
        if (q < k) {
          if constexpr (kDrop)  // behind the fence above: the slot's owner has rewritten it
            o[i] = stage_v[q];
          else
            o[i] = x[i];
        }
        ++q;
      }
    }
    float* dst = dense.p + (size_t)row * dense.stride;
    const int j0 = lane * 4;
    // one float4 where every row starts 16-B aligned (wave-uniform), scalars otherwise
    if ((D & 3) == 0 && ((reinterpret_cast<uintptr_t>(dense.p) | (uintptr_t)(4 * dense.stride)) & 15) == 0) {
      if (j0 < D) *reinterpret_cast<float4*>(dst + j0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (j0 + i < D) dst[j0 + i] = o[i];
    }
  }
  // the next row's staging writes follow these reads in the wave's in-order LDS queue
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int kTopkWalk = 4;         // top-byte bins walked with ballots before the histogram

// Exact top-k selection of one row held as 4 features per lane (x[i] = feature 4 * lane + i):
// sel[i] = whether (lane, i) is among the k largest, ties at the k-th value to the lowest
// feature index. Radix select of the k-th largest key in 8-bit digits: the top byte by a ballot
// walk, the rest through the wave's private 256-bin LDS histogram `hist` (ds_add_u32) with DPP
// suffix sums; stops as soon as the threshold bin holds exactly the keys still needed.
__device__ __forceinline__ void exact_select(const float x[4], const bool valid[4], int k,
                                             uint32_t* hist, int lane, bool sel[4]) {
  uint32_t u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = order_key(x[i]);

  uint32_t prefix = 0, pmask = 0;
  uint32_t need = (uint32_t)k;  // still to select among the keys matching the prefix
  bool whole_bin = false;       // the last fixed digit's bin holds exactly `need` keys
  // Top byte (sign + exponent) by a descending walk over bins with ballots: float keys
  // share few top bytes, so a histogram pass piles its LDS atomics onto 2-5 addresses
  // (same-address ds_add serialises); the walk counts bin top, top-1, ... and stops at
  // the bin holding the k-th largest key (usually 2 steps). Falls back to the
  // histogram after kTopkWalk bins.
  int first_shift = 24;
  {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) m = max(m, valid[i] ? u[i] : 0u);
    m = wave_umax(m);
    const int top = (int)(m >> 24);
    uint32_t left = need;
    for (int it = 0; it < kTopkWalk && top - it >= 0; ++it) {
      const uint32_t b = (uint32_t)(top - it);
      uint32_t cnt = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) cnt += (uint32_t)wave_count(valid[i] && (u[i] >> 24) == b);
      if (cnt >= left) {
        prefix = b << 24;
        pmask = 0xff000000u;
        need = left;
        whole_bin = cnt == left;
        first_shift = 16;
        break;
      }
      left -= cnt;
    }
  }
#pragma unroll
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (shift > first_shift || whole_bin) continue;  // wave-uniform
    reinterpret_cast<uint4*>(hist)[lane] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (valid[i] && (u[i] & pmask) == prefix)
        __hip_atomic_fetch_add(&hist[(u[i] >> shift) & 255u], 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WAVEFRONT);
    const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];  // bins 4*lane .. +3
    const uint32_t lsum = h.x + h.y + h.z + h.w;
    const uint32_t pre = wave_prefix_sum(lsum);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)pre, kWave - 1);
    const uint32_t ge3 = total - pre + h.w;  // keys in bins >= 4*lane + 3
    const uint32_t ge2 = ge3 + h.z, ge1 = ge2 + h.y, ge0 = ge1 + h.x;
    // digit of the need-th largest key: the largest bin b with #(bins >= b) >= need
    const uint64_t m = __ballot(ge0 >= need);  // a prefix of lanes, lane 0 always in it
    const int ls = 63 - __builtin_clzll(m);
    uint32_t d, above, inbin;
    if (ge3 >= need) { d = 3; above = ge3 - h.w; inbin = h.w; }
    else if (ge2 >= need) { d = 2; above = ge3; inbin = h.z; }
    else if (ge1 >= need) { d = 1; above = ge2; inbin = h.y; }
    else { d = 0; above = ge1; inbin = h.x; }
    d = (uint32_t)__builtin_amdgcn_readlane((int)(4 * lane + d), ls);
    above = (uint32_t)__builtin_amdgcn_readlane((int)above, ls);
    inbin = (uint32_t)__builtin_amdgcn_readlane((int)inbin, ls);
    need -= above;
    prefix |= d << shift;
    pmask |= 255u << shift;
    if (inbin == need) {  // uniform: every key of the bin is selected, no ties to break
      whole_bin = true;
      break;
    }
  }

  if (whole_bin) {
    // exactly k keys have their fixed high bits >= the prefix
#pragma unroll
    for (int i = 0; i < 4; ++i) sel[i] = valid[i] && (u[i] & pmask) >= prefix;
  } else {
    const uint32_t T = prefix;  // the k-th largest key; `need` of its ties are selected
    bool gt[4], eq[4];
    uint64_t meq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gt[i] = valid[i] && u[i] > T;
      eq[i] = valid[i] && u[i] == T;
      meq[i] = __ballot(eq[i]);
    }
    // Ties at the threshold: the lowest feature indices win.
    int rank = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) rank += (int)lanes_below(meq[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sel[i] = gt[i] || (eq[i] && rank < (int)need);
      rank += eq[i] ? 1 : 0;
    }
  }
}

}  // namespace maxk
