// GATv2 attention scored on MaxK features (include/maxk_hip.h, "MaxK GATv2 attention"). With
// xs = MaxK(fs) the GATv2 score of edge u -> v splits into a part that depends on v alone, which
// the softmax over v's in-edges removes, and k gathered terms:
//
//   D[h, e] = sum_{l: hd(s) = h} attn[s] (lrelu(x + fd[v, s]) - lrelu(fd[v, s]))
//             x = sp_data[u, l], s = sp_index[u, l], hd(s) = s / F
//
//   score forward    D [H, E] from the CSR, the tables, fd [num_rows, D] and attn [D]
//   softmax          maxk_edge_softmax_* over every head of [H, E] (edge_softmax.h, as it is)
//   backward, rows   grad_fd[v, s] = sum_e g[hd(s), e] attn[s] (lrelu'(x + fd) - lrelu'(fd))
//                    grad_attn[s]  = sum_{e, l} g[hd(s), e] (lrelu(x + fd) - lrelu(fd))
//   backward, cols   grad_sp[u, l] = attn[s] sum_{e in out(u)} g[hd(s), e] lrelu'(x + fd[row(e), s])
//
// No plan, no global atomics, nothing allocated. All three score kernels are gather-bound (k
// slots of 5 bytes per edge against a handful of flops), so there is no matrix instruction here.
//
// Work split: the tile walk of lane_groups.h, as it is. A work-group of 4 waves owns 16 rows
// (columns); a row of at most 16 edges is served by one lane group of LP = lanes(k) lanes, one of
// at most 512 by a wave, a longer one by the work-group. An edge is one lane group's: lane `sub`
// holds slot sub (and sub + 64 i above k = 64).
//
// Forward: attn sits in LDS for the work-group; whoever serves a row stages {fd[v, s],
// lrelu(fd[v, s])} as one float2 per feature in an LDS row of its own (one ds_read_b64 per slot),
// so fd is read once per destination row and every gather by selector is an LDS access. The
// lanes' terms are reduced per head by the reduce-scatter butterfly of heads_bwd_kernel over HP
// head places, which leaves head bitrev(sub) in lane sub < HP: every (h, e) is stored once.
// Backward, rows: the same staging; the terms of grad_fd go into an LDS row per destination row
// with ds_add_f32 (a short row's group, a medium row's wave, one row per wave of a hub combined
// as (w0 + w1) + (w2 + w3)) and the row is stored once, zeros included. The terms of grad_attn go
// into one LDS row per wave for the whole life of the work-group, which walks tiles blockIdx.x,
// blockIdx.x + gridDim.x, ... and leaves one [D] partial in the caller's scratch; a second kernel
// adds the partials in a fixed order. Backward, columns: a lane keeps its slot's x, s, attn[s] and
// partial sum in registers across the column's out-edges (heads_bwd_kernel's shape) and gathers
// fd[r, s] and g[hd(s), e] from memory.
#include "common.h"
#include "edge_softmax.h"
#include "variants_gatv2.h"

namespace maxk_v2 {

using maxk::check_ranges;
// the softmax's geometry and device functions (edge_softmax.h)
using maxk::es_bwd_hub;
using maxk::es_bwd_medium;
using maxk::es_bwd_regs;
using maxk::es_fwd_hub;
using maxk::es_fwd_medium;
using maxk::es_fwd_regs;
using maxk::EsArray;
using maxk::EsNoPost;
using maxk::kEsGroup;
using maxk::kEsMediumMax;
using maxk::kEsShortMax;
using maxk::kEsShortSlots;
using maxk::kEsThreads;
using maxk::kEsTileRows;
using maxk::kEsWaveRows;
using maxk::kEsWaves;
using maxk::clampi;
using maxk::kWave;
using maxk::Range;
using maxk::row_segment;
using maxk::set_error;
using maxk::lg::wave_lds_sync;

constexpr int kEdgesInFlight = 2;

// LDS rows that the serving lane groups (at most one per row of the tile) can hold at once
constexpr int stage_slots(int lp) {
  return lg::kThreads / lp < lg::kTile ? lg::kThreads / lp : lg::kTile;
}
// then one row per wave (medium rows, and the hub pass)
constexpr int lds_rows(int lp) { return stage_slots(lp) + lg::kWaves; }

__device__ __forceinline__ void lds_add(float* p, float v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // ds_add_f32
}

__device__ __forceinline__ float lrelu(float t, float slope) { return t > 0.f ? t : slope * t; }

// The head that lane `sub` < HP holds after the reduce-scatter (heads_aggregate.hip).
template <int HP>
__device__ __forceinline__ int held_head(int sub) {
  int h = 0;
#pragma unroll
  for (int t = 0; (1 << t) < HP; ++t) h |= ((sub >> t) & 1) * (HP >> (t + 1));
  return h;
}

// The slots of column c that lane `sub` holds: selector (clamped), head and value.
template <int LP, int S>
struct Slots {
  uint32_t s[S];
  int h[S];
  float x[S];
  bool on[S];
  __device__ __forceinline__ void load(const float* data, int64_t ds, const uint8_t* sel,
                                       int64_t is, int64_t c, int sub, int k, int D,
                                       uint32_t magic) {
    const uint32_t sel_hi = (uint32_t)(D - 1);
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const int l = sub + LP * i;
      on[i] = l < k;
      const uint32_t raw = on[i] ? sel[c * is + l] : 0u;
      s[i] = raw < sel_hi ? raw : sel_hi;
      h[i] = heads_head_of((int)s[i], magic);
      x[i] = on[i] ? data[c * ds + l] : 0.f;
    }
  }
};

// ---------------------------------------------------------------------------- score forward
struct FwdArgs {
  const int32_t* ptr;
  const int32_t* idx;
  const float* data;
  int64_t ds;
  const uint8_t* sel;
  int64_t is;
  const float* fd;
  int64_t fs;
  const float* attn;
  float slope;
  float* out;
  int32_t H, num_rows, num_cols;
  int64_t E;
  int32_t D, k;
  uint32_t magic;
};

// Edges first, first + step, ... of the row at [b, b + n), whose {fd, lrelu(fd)} is `row`.
template <int LP, int HP, int S>
__device__ __forceinline__ void fwd_edges(const FwdArgs& a, const float2* row, const float* attn,
                                          int64_t b, int32_t n, int first, int step, int sub) {
  constexpr int U = kEdgesInFlight;
  const int32_t col_hi = a.num_cols - 1;
  const int mine = held_head<HP>(sub);
  const bool writer = sub < HP && mine < a.H;
  for (int64_t j0 = first; j0 < n; j0 += (int64_t)step * U) {
    int64_t e[U];
    bool ok[U];
    Slots<LP, S> t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * step;
      ok[u] = j < n;
      e[u] = b + (ok[u] ? j : (int64_t)n - 1);  // an edge of the row either way
      t[u].load(a.data, a.ds, a.sel, a.is, clampi(a.idx[e[u]], col_hi), sub, a.k, a.D, a.magic);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float v[HP];
#pragma unroll
      for (int q = 0; q < HP; ++q) v[q] = 0.f;
#pragma unroll
      for (int i = 0; i < S; ++i) {
        const float2 r = row[t[u].s[i]];
        const float term = attn[t[u].s[i]] * (lrelu(t[u].x[i] + r.x, a.slope) - r.y);
#pragma unroll
        for (int q = 0; q < HP; ++q)
          if (t[u].on[i] && t[u].h[i] == q) v[q] = v[q] + term;
      }
      // reduce-scatter over the HP lanes that share sub / HP: each stage halves the heads a lane
      // holds and adds the partner's terms of the half it keeps
#pragma unroll
      for (int st = 0; (1 << st) < HP; ++st) {
        const int half = HP >> (st + 1);
        const bool up = (sub >> st) & 1;
#pragma unroll
        for (int q = 0; q < half; ++q) {
          const float send = up ? v[q] : v[q + half];
          const float keep = up ? v[q + half] : v[q];
          v[q] = keep + __shfl_xor(send, 1 << st, kWave);
        }
      }
      float tot = v[0];
#pragma unroll
      for (int m = HP; m < LP; m <<= 1) tot = tot + __shfl_xor(tot, m, kWave);
      if (writer && ok[u]) a.out[(int64_t)mine * a.E + e[u]] = tot;
    }
  }
}

template <int LP, int HP>
__global__ __launch_bounds__(lg::kThreads) void gatv2_score_fwd_kernel(const FwdArgs a) {
  static_assert(LP >= HP, "the reduce-scatter ends with one head per lane");
  extern __shared__ float lds[];  // attn [D], then lds_rows(LP) rows of D float2
  constexpr int S = lg::lane_slots(LP);
  constexpr int NS = stage_slots(LP);
  const lg::Place<LP> p{};
  const int D = a.D;
  const float slope = a.slope;
  float* attn = lds;
  float2* stage = reinterpret_cast<float2*>(lds + D);
  const int64_t row0 = (int64_t)blockIdx.x * lg::kTile;

  for (int j = p.tid; j < D; j += lg::kThreads) attn[j] = a.attn[j];
  __syncthreads();

  auto fill = [&](float2* dst, int64_t row, int first, int step) {
    for (int j = first; j < D; j += step) {
      const float f = a.fd[row * a.fs + j];
      dst[j] = make_float2(f, lrelu(f, slope));
    }
  };

  // a group with a row has gid < kTile, so gid < NS
  lg::short_rows(p, a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
    if (n == 0) return;
    float2* mine = stage + p.gid * D;
    fill(mine, row, p.sub, LP);
    wave_lds_sync();
    fwd_edges<LP, HP, S>(a, mine, attn, b, n, 0, 1, p.sub);
    wave_lds_sync();
  });

  lg::medium_rows(p, a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
    float2* mine = stage + (NS + p.wave) * D;
    fill(mine, row, p.lane, kWave);
    wave_lds_sync();
    fwd_edges<LP, HP, S>(a, mine, attn, b, n, p.g, p.G, p.sub);
    wave_lds_sync();
  });

  lg::hub_rows(a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
    float2* mine = stage + NS * D;
    __syncthreads();  // wave 0 is done with this row, and the tile's previous hub was served
    fill(mine, row, p.tid, lg::kThreads);
    __syncthreads();
    fwd_edges<LP, HP, S>(a, mine, attn, b, n, p.gid, p.NG, p.sub);
  });
}

// --------------------------------------------------------------------------- backward, rows
struct RowsArgs {
  const int32_t* ptr;
  const int32_t* idx;
  const float* data;
  int64_t ds;
  const uint8_t* sel;
  int64_t is;
  const float* fd;
  int64_t fs;
  const float* attn;
  float slope;
  const float* g;    // grad_logits [H, E]
  float* grad_fd;    // [num_rows, D]
  float* partial;    // [gridDim.x, D]
  int32_t num_rows, num_cols;
  int64_t E;
  int32_t D, k;
  uint32_t magic;
  int32_t tiles;
};

// Edges first, first + step, ... of the row at [b, b + n) whose fd is `fdrow`: their terms of
// grad_fd into acc, of grad_attn into gat (LDS rows of D floats).
template <int LP, int S>
__device__ __forceinline__ void rows_edges(const RowsArgs& a, const float* fdrow,
                                           const float* attn, float* acc, float* gat, int64_t b,
                                           int32_t n, int first, int step, int sub) {
  constexpr int U = kEdgesInFlight;
  const int32_t col_hi = a.num_cols - 1;
  const float slope = a.slope;
  for (int64_t j0 = first; j0 < n; j0 += (int64_t)step * U) {
    int64_t e[U];
    bool ok[U];
    Slots<LP, S> t[U];
    float gv[U][S];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * step;
      ok[u] = j < n;
      e[u] = b + (ok[u] ? j : (int64_t)n - 1);
      t[u].load(a.data, a.ds, a.sel, a.is, clampi(a.idx[e[u]], col_hi), sub, a.k, a.D, a.magic);
#pragma unroll
      for (int i = 0; i < S; ++i) gv[u][i] = a.g[(int64_t)t[u].h[i] * a.E + e[u]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < S; ++i) {
        if (!(ok[u] && t[u].on[i])) continue;
        const uint32_t s = t[u].s[i];
        const float f = fdrow[s];
        const float z = t[u].x[i] + f;
        lds_add(gat + s, gv[u][i] * (lrelu(z, slope) - lrelu(f, slope)));
        // lrelu'(z) - lrelu'(f): nothing where both are on one side of zero
        if ((z > 0.f) != (f > 0.f))
          lds_add(acc + s, (gv[u][i] * attn[s]) * (z > 0.f ? 1.f - slope : slope - 1.f));
      }
  }
}

template <int LP>
__global__ __launch_bounds__(lg::kThreads) void gatv2_score_bwd_rows_kernel(const RowsArgs a) {
  // attn [D], grad_attn of the waves [4][D], then lds_rows(LP) rows of fd and as many of grad_fd
  extern __shared__ float lds[];
  constexpr int S = lg::lane_slots(LP);
  constexpr int NS = stage_slots(LP);
  const lg::Place<LP> p{};
  const int D = a.D;
  float* attn = lds;
  float* gat = lds + D;
  float* stage = gat + lg::kWaves * D;
  float* accs = stage + lds_rows(LP) * D;
  float* wgat = gat + p.wave * D;

  for (int j = p.tid; j < D; j += lg::kThreads) attn[j] = a.attn[j];
  for (int j = p.tid; j < lg::kWaves * D; j += lg::kThreads) gat[j] = 0.f;
  __syncthreads();

  for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const int64_t row0 = tile * lg::kTile;

    lg::short_rows(p, a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
      float* fdrow = stage + p.gid * D;
      float* acc = accs + p.gid * D;
      for (int j = p.sub; j < D; j += LP) {
        fdrow[j] = a.fd[row * a.fs + j];
        acc[j] = 0.f;
      }
      wave_lds_sync();
      rows_edges<LP, S>(a, fdrow, attn, acc, wgat, b, n, 0, 1, p.sub);
      wave_lds_sync();
      for (int j = p.sub; j < D; j += LP) a.grad_fd[row * D + j] = acc[j];
      wave_lds_sync();
    });

    lg::medium_rows(p, a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
      float* fdrow = stage + (NS + p.wave) * D;
      float* acc = accs + (NS + p.wave) * D;
      for (int j = p.lane; j < D; j += kWave) {
        fdrow[j] = a.fd[row * a.fs + j];
        acc[j] = 0.f;
      }
      wave_lds_sync();
      rows_edges<LP, S>(a, fdrow, attn, acc, wgat, b, n, p.g, p.G, p.sub);
      wave_lds_sync();
      for (int j = p.lane; j < D; j += kWave) a.grad_fd[row * D + j] = acc[j];
      wave_lds_sync();
    });

    lg::hub_rows(a.ptr, row0, a.num_rows, a.E, [&](int64_t row, int64_t b, int32_t n) {
      float* fdrow = stage + NS * D;
      float* acc = accs + NS * D;  // the four waves' rows
      __syncthreads();  // every wave is done with its own rows, the previous hub was stored
      for (int j = p.tid; j < D; j += lg::kThreads) fdrow[j] = a.fd[row * a.fs + j];
      for (int j = p.tid; j < lg::kWaves * D; j += lg::kThreads) acc[j] = 0.f;
      __syncthreads();
      rows_edges<LP, S>(a, fdrow, attn, acc + p.wave * D, wgat, b, n, p.gid, p.NG, p.sub);
      __syncthreads();
      for (int j = p.tid; j < D; j += lg::kThreads)
        a.grad_fd[row * D + j] = (acc[j] + acc[D + j]) + (acc[2 * D + j] + acc[3 * D + j]);
    });
    __syncthreads();  // the rows of LDS are free for the next tile
  }

  __syncthreads();
  for (int j = p.tid; j < D; j += lg::kThreads)
    a.partial[(int64_t)blockIdx.x * D + j] =
        (gat[j] + gat[D + j]) + (gat[2 * D + j] + gat[3 * D + j]);
}

// grad_attn[s] = the partials' sum: wave w adds partials w, w + 4, ... in order, the four waves
// meet as (w0 + w1) + (w2 + w3). One work-group per 64 features.
__global__ __launch_bounds__(lg::kThreads) void gatv2_attn_reduce_kernel(
    const float* __restrict__ partial, int32_t parts, float* __restrict__ grad_attn, int32_t D) {
  __shared__ float red[lg::kWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int s = blockIdx.x * kWave + lane;
  float v = 0.f;
  if (s < D)
    for (int32_t t = wave; t < parts; t += lg::kWaves) v = v + partial[(int64_t)t * D + s];
  red[wave][lane] = v;
  __syncthreads();
  if (wave == 0 && s < D)
    grad_attn[s] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// ------------------------------------------------------------------------ backward, columns
struct ColsArgs {
  const int32_t* ptr_t;
  const int32_t* idx_t;
  const int32_t* order;
  const float* data;
  int64_t ds;
  const uint8_t* sel;
  int64_t is;
  const float* fd;
  int64_t fs;
  const float* attn;
  float slope;
  const float* g;  // grad_logits [H, E]
  float* grad_sp;  // [num_cols, k]
  int32_t num_rows, num_cols;
  int64_t E;
  int32_t D, k;
  uint32_t magic;
};

// Transposed entries first, first + step, ... of the column at [b, b + n) whose slots are t: adds
// g[hd(s), e] lrelu'(x + fd[r, s]) into gsp[i].
template <int LP, int S>
__device__ __forceinline__ void cols_edges(const ColsArgs& a, const Slots<LP, S>& t, int64_t b,
                                           int32_t n, int first, int step, float (&gsp)[S]) {
  constexpr int U = kEdgesInFlight;
  const int32_t edge_hi = (int32_t)(a.E - 1), row_hi = a.num_rows - 1;
  const float slope = a.slope;
  for (int64_t j0 = first; j0 < n; j0 += (int64_t)step * U) {
    bool ok[U];
    float f[U][S], gv[U][S];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * step;
      ok[u] = j < n;
      const int64_t jj = b + (ok[u] ? j : (int64_t)n - 1);
      const int64_t e = clampi(a.order[jj], edge_hi);
      const int64_t r = clampi(a.idx_t[jj], row_hi);
#pragma unroll
      for (int i = 0; i < S; ++i) {
        f[u][i] = a.fd[r * a.fs + t.s[i]];
        gv[u][i] = a.g[(int64_t)t.h[i] * a.E + e];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < S; ++i)
        if (ok[u] && t.on[i])
          gsp[i] = gsp[i] + (t.x[i] + f[u][i] > 0.f ? gv[u][i] : slope * gv[u][i]);
  }
}

template <int LP>
__global__ __launch_bounds__(lg::kThreads) void gatv2_score_bwd_cols_kernel(const ColsArgs a) {
  constexpr int S = lg::lane_slots(LP);
  __shared__ float red[lg::kWaves][maxk::kMaxDim];
  const lg::Place<LP> p{};
  const int k = a.k;
  const int64_t col0 = (int64_t)blockIdx.x * lg::kTile;

  // the column's slots and attn[s] stay in registers across its entries
  auto serve = [&](int64_t col, int64_t b, int32_t n, int first, int step, float (&gsp)[S]) {
    Slots<LP, S> t;
    t.load(a.data, a.ds, a.sel, a.is, col, p.sub, k, a.D, a.magic);
    cols_edges<LP, S>(a, t, b, n, first, step, gsp);
#pragma unroll
    for (int i = 0; i < S; ++i) gsp[i] = a.attn[t.s[i]] * gsp[i];
  };

  lg::short_rows(p, a.ptr_t, col0, a.num_cols, a.E, [&](int64_t col, int64_t b, int32_t n) {
    float gsp[S] = {};
    serve(col, b, n, 0, 1, gsp);
    lg::store_group(p, gsp, k, a.grad_sp, col);
  });

  lg::medium_rows(p, a.ptr_t, col0, a.num_cols, a.E, [&](int64_t col, int64_t b, int32_t n) {
    float gsp[S] = {};
    serve(col, b, n, p.g, p.G, gsp);
    lg::reduce_wave_and_store(p, gsp, k, a.grad_sp, col);
  });

  lg::hub_rows(a.ptr_t, col0, a.num_cols, a.E, [&](int64_t col, int64_t b, int32_t n) {
    float gsp[S] = {};
    serve(col, b, n, p.gid, p.NG, gsp);
    lg::reduce_block_and_store(p, gsp, k, a.grad_sp, col, red);
  });
}

// ------------------------------------------------------------------------ softmax, per head
// The bodies of edge_softmax_fwd_kernel / edge_softmax_bwd_kernel (edge_softmax.hip) on head
// blockIdx.y of the head-major arrays: the same device functions on the same values, so head h is
// the single-head call on row h bit for bit (edge_softmax.h turns contraction off for the rest of
// this file, as edge_softmax.hip does for its own).

__global__ __launch_bounds__(kEsThreads) void edge_softmax_fwd_heads_kernel(
    const int32_t* __restrict__ ptr, const float* __restrict__ logits_all,
    float* __restrict__ out_all, int32_t num_rows, int64_t E) {
  __shared__ float red[2 * kEsWaves];
  const float* __restrict__ logits = logits_all + (int64_t)blockIdx.y * E;
  float* __restrict__ out = out_all + (int64_t)blockIdx.y * E;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kEsTileRows;

  int64_t b;
  int32_t n;
  row_segment(ptr, row0 + wave * kEsWaveRows + lane / kEsGroup, num_rows, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  if (__ballot(ns > 0) != 0) {
    const int64_t bs = ns > 0 ? b : 0;
    es_fwd_regs<kEsGroup, kEsShortSlots>(EsArray{logits + bs}, out + bs, ns, lane % kEsGroup);
  }
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    es_fwd_medium(EsArray{logits + bg}, out + bg, ng, lane);
  }
  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    row_segment(ptr, row0 + r, num_rows, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    es_fwd_hub(EsArray{logits + bh}, out + bh, nh, tid, lane, wave, red);
  }
}

__global__ __launch_bounds__(kEsThreads) void edge_softmax_bwd_heads_kernel(
    const int32_t* __restrict__ ptr, const float* __restrict__ y_all,
    const float* __restrict__ gy_all, float* __restrict__ out_all, int32_t num_rows, int64_t E) {
  __shared__ float red[kEsWaves];
  const float* __restrict__ y = y_all + (int64_t)blockIdx.y * E;
  const float* __restrict__ gy = gy_all + (int64_t)blockIdx.y * E;
  float* __restrict__ out = out_all + (int64_t)blockIdx.y * E;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kEsTileRows;

  int64_t b;
  int32_t n;
  row_segment(ptr, row0 + wave * kEsWaveRows + lane / kEsGroup, num_rows, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  if (__ballot(ns > 0) != 0) {
    const int64_t bs = ns > 0 ? b : 0;
    es_bwd_regs<kEsGroup, kEsShortSlots>(y + bs, gy + bs, out + bs, ns, lane % kEsGroup,
                                         EsNoPost{});
  }
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    es_bwd_medium(y + bg, gy + bg, out + bg, ng, lane, EsNoPost{});
  }
  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    row_segment(ptr, row0 + r, num_rows, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    es_bwd_hub(y + bh, gy + bh, out + bh, nh, tid, lane, wave, red, EsNoPost{});
    __syncthreads();  // red is free for the tile's next hub
  }
}

// ------------------------------------------------------------------------------ entry points
static int32_t partial_count(int32_t num_rows) {
  const int64_t tiles = ((int64_t)num_rows + lg::kTile - 1) / lg::kTile;
  return (int32_t)(tiles < kGatv2MaxPartials ? tiles : kGatv2MaxPartials);
}

static int64_t scratch_bytes(int32_t num_rows, int32_t D) {
  if (num_rows < 0 || D < 1 || D > maxk::kMaxDim) return -1;
  return 4 * (int64_t)D * partial_count(num_rows);
}

// sizes, k, heads, strides and the slope shared by the three score calls; strides are resolved
// (0: the row width)
static int check_shape(const std::string& w, int32_t H, int32_t num_rows, int32_t num_cols,
                       int64_t E, int32_t D, int32_t k, int64_t& ds, int64_t& is, int64_t& fs,
                       float slope) {
  return lg::check_shape(w, num_rows, num_cols, E, D, k, is, [&]() -> int {
    MAXK_CHECK_ARG(H >= 1 && D % H == 0, w + "num_heads must be >= 1 and divide dim_origin");
    if (D % 4 != 0) {
      set_error(w + "dim_origin must be a multiple of 4");
      return MAXK_ERR_UNSUPPORTED;
    }
    if (H > kGatv2MaxHeads) {
      set_error(w + "num_heads above 16 is not supported");
      return MAXK_ERR_UNSUPPORTED;
    }
    MAXK_CHECK_ARG(slope == slope && slope - slope == 0.f, w + "negative_slope must be finite");
    if (ds == 0) ds = k;
    MAXK_CHECK_ARG(ds >= k, w + "data_stride must be >= k (0: k)");
    if (fs == 0) fs = D;
    MAXK_CHECK_ARG(fs >= D, w + "fd_stride must be >= dim_origin (0: dim_origin)");
    return MAXK_OK;
  });
}

static int score_forward(const int32_t* ptr, const int32_t* idx, const float* sp_data, int64_t ds,
                         const uint8_t* sp_index, int64_t is, const float* fd, int64_t fs,
                         const float* attn, float slope, float* logits, int32_t H, int32_t N,
                         int32_t NC, int64_t E, int32_t D, int32_t k, void* stream) {
  const std::string w("maxk_gatv2_score_forward: ");
  int rc = check_shape(w, H, N, NC, E, D, k, ds, is, fs, slope);
  if (rc != MAXK_OK) return rc;
  if (N == 0 || E == 0) return MAXK_OK;  // logits has no element
  const Range ins[6] = {{ptr, 4 * ((int64_t)N + 1)},
                        {idx, 4 * E},
                        {sp_data, 4 * ((int64_t)(NC - 1) * ds + k)},
                        {sp_index, (int64_t)(NC - 1) * is + k},
                        {fd, 4 * ((int64_t)(N - 1) * fs + D)},
                        {attn, 4 * (int64_t)D}};
  const Range outs[1] = {{logits, 4 * H * E}};
  rc = check_ranges(w, ins, 6, outs, 1);
  if (rc != MAXK_OK) return rc;
  const FwdArgs a{ptr, idx, sp_data, ds, sp_index, is, fd, fs, attn, slope, logits, H, N, NC, E,
                  D, k, heads_magic(D / H)};
  if (int e = maxk::dispatch_variant(
          kScoreFwdVariants, select_score_fwd_variant(k, H), [&](auto i) -> int {
            constexpr ScoreFwdVariant v = kScoreFwdVariants[decltype(i)::value];
            const size_t lds = sizeof(float) * (size_t)D * (1 + 2 * lds_rows(v.lp));
            hipLaunchKernelGGL((gatv2_score_fwd_kernel<v.lp, v.hp>), lg::tile_grid(N),
                               dim3(lg::kThreads), lds, (hipStream_t)stream, a);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_gatv2_score_forward launch");
  return MAXK_OK;
}

static int score_backward_rows(const int32_t* ptr, const int32_t* idx, const float* sp_data,
                               int64_t ds, const uint8_t* sp_index, int64_t is, const float* fd,
                               int64_t fs, const float* attn, float slope, const float* g,
                               float* grad_fd, float* grad_attn, void* scratch, int64_t sbytes,
                               int32_t H, int32_t N, int32_t NC, int64_t E, int32_t D, int32_t k,
                               void* stream) {
  const std::string w("maxk_gatv2_score_backward_rows: ");
  int rc = check_shape(w, H, N, NC, E, D, k, ds, is, fs, slope);
  if (rc != MAXK_OK) return rc;
  const int32_t parts = partial_count(N);
  const int64_t need = scratch_bytes(N, D);
  MAXK_CHECK_ARG(sbytes >= need, w + "scratch_bytes is below maxk_gatv2_scratch_bytes");
  MAXK_CHECK_ARG((reinterpret_cast<uintptr_t>(scratch) & 3) == 0,
                 w + "scratch must be 4-B aligned");
  // without edges the tables and grad_logits are not read: every row is empty
  const Range ins[8] = {{ptr, N ? 4 * ((int64_t)N + 1) : 0},
                        {idx, 4 * E},
                        {sp_data, E ? 4 * ((int64_t)(NC - 1) * ds + k) : 0},
                        {sp_index, E ? (int64_t)(NC - 1) * is + k : 0},
                        {fd, N ? 4 * ((int64_t)(N - 1) * fs + D) : 0},
                        {attn, N ? 4 * (int64_t)D : 0},
                        {g, 4 * H * E}};
  const Range outs[3] = {{grad_fd, 4 * (int64_t)N * D}, {grad_attn, 4 * (int64_t)D},
                         {scratch, need}};
  rc = check_ranges(w, ins, 7, outs, 3);
  if (rc != MAXK_OK) return rc;
  if (N > 0) {
    const RowsArgs a{ptr, idx, sp_data, ds, sp_index, is, fd, fs, attn, slope, g, grad_fd,
                     (float*)scratch, N, NC, E, D, k, heads_magic(D / H),
                     (int32_t)(((int64_t)N + lg::kTile - 1) / lg::kTile)};
    if (int e = maxk::dispatch_variant(
            kScoreRowsVariants, select_score_rows_variant(k), [&](auto i) -> int {
              constexpr int LP = kScoreRowsVariants[decltype(i)::value].lp;
              const size_t lds =
                  sizeof(float) * (size_t)D * (1 + lg::kWaves + 2 * lds_rows(LP));
              hipLaunchKernelGGL(gatv2_score_bwd_rows_kernel<LP>, dim3((unsigned)parts),
                                 dim3(lg::kThreads), lds, (hipStream_t)stream, a);
              return MAXK_OK;
            }))
      return e;
  }
  hipLaunchKernelGGL(gatv2_attn_reduce_kernel, dim3((unsigned)((D + kWave - 1) / kWave)),
                     dim3(lg::kThreads), 0, (hipStream_t)stream, (const float*)scratch, parts,
                     grad_attn, D);
  MAXK_LAUNCH_CHECK("maxk_gatv2_score_backward_rows launch");
  return MAXK_OK;
}

static int score_backward_cols(const int32_t* ptr_t, const int32_t* idx_t, const int32_t* order,
                               const float* sp_data, int64_t ds, const uint8_t* sp_index,
                               int64_t is, const float* fd, int64_t fs, const float* attn,
                               float slope, const float* g, float* grad_sp, int32_t H, int32_t N,
                               int32_t NC, int64_t E, int32_t D, int32_t k, void* stream) {
  const std::string w("maxk_gatv2_score_backward_cols: ");
  int rc = check_shape(w, H, N, NC, E, D, k, ds, is, fs, slope);
  if (rc != MAXK_OK) return rc;
  if (NC == 0) return MAXK_OK;
  const Range ins[8] = {{ptr_t, 4 * ((int64_t)NC + 1)},
                        {idx_t, 4 * E},
                        {order, 4 * E},
                        {sp_data, 4 * ((int64_t)(NC - 1) * ds + k)},
                        {sp_index, (int64_t)(NC - 1) * is + k},
                        {fd, E ? 4 * ((int64_t)(N - 1) * fs + D) : 0},
                        {attn, 4 * (int64_t)D},
                        {g, 4 * H * E}};
  const Range outs[1] = {{grad_sp, 4 * (int64_t)NC * k}};
  rc = check_ranges(w, ins, 8, outs, 1);
  if (rc != MAXK_OK) return rc;
  const ColsArgs a{ptr_t, idx_t, order, sp_data, ds, sp_index, is, fd, fs, attn, slope, g,
                   grad_sp, N, NC, E, D, k, heads_magic(D / H)};
  if (int e = maxk::dispatch_variant(
          kScoreColsVariants, select_score_cols_variant(k), [&](auto i) -> int {
            constexpr int LP = kScoreColsVariants[decltype(i)::value].lp;
            hipLaunchKernelGGL(gatv2_score_bwd_cols_kernel<LP>, lg::tile_grid(NC),
                               dim3(lg::kThreads), 0, (hipStream_t)stream, a);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_gatv2_score_backward_cols launch");
  return MAXK_OK;
}

// Checks of the two softmax calls: `ins` are the nin f32 [H, E] inputs; run: there is something
// to launch.
static int softmax_check(const std::string& w, const int32_t* ptr, const float* const* ins,
                         int nin, const float* out, int32_t H, int32_t N, int64_t E, bool& run) {
  run = false;
  MAXK_CHECK_ARG(N >= 0 && E >= 0 && E <= (int64_t)INT32_MAX, w + "sizes out of range");
  MAXK_CHECK_ARG(H >= 1, w + "num_heads must be >= 1");
  MAXK_CHECK_ARG(H <= 65535, w + "num_heads beyond the grid's 65535");
  if (E == 0 || N == 0) return MAXK_OK;
  Range in[3] = {{ptr, 4 * ((int64_t)N + 1)}, {nullptr, 0}, {nullptr, 0}};
  for (int i = 0; i < nin; ++i) in[1 + i] = {ins[i], 4 * H * E};
  const Range outs[1] = {{out, 4 * H * E}};
  const int rc = check_ranges(w, in, 1 + nin, outs, 1);
  run = rc == MAXK_OK;
  return rc;
}

}  // namespace maxk_v2

extern "C" int maxk_gatv2_score_forward(const int32_t* ptr, const int32_t* idx,
                                        const float* sp_data, int64_t data_stride,
                                        const uint8_t* sp_index, int64_t index_stride,
                                        const float* fd, int64_t fd_stride, const float* attn,
                                        float negative_slope, float* logits, int32_t num_heads,
                                        int32_t num_rows, int32_t num_cols, int64_t num_edges,
                                        int32_t dim_origin, int32_t dim_k, void* stream) {
  return maxk_v2::score_forward(ptr, idx, sp_data, data_stride, sp_index, index_stride, fd,
                                fd_stride, attn, negative_slope, logits, num_heads, num_rows,
                                num_cols, num_edges, dim_origin, dim_k, stream);
}

extern "C" int maxk_gatv2_score_backward_rows(
    const int32_t* ptr, const int32_t* idx, const float* sp_data, int64_t data_stride,
    const uint8_t* sp_index, int64_t index_stride, const float* fd, int64_t fd_stride,
    const float* attn, float negative_slope, const float* grad_logits, float* grad_fd,
    float* grad_attn, void* scratch, int64_t scratch_bytes, int32_t num_heads, int32_t num_rows,
    int32_t num_cols, int64_t num_edges, int32_t dim_origin, int32_t dim_k, void* stream) {
  return maxk_v2::score_backward_rows(ptr, idx, sp_data, data_stride, sp_index, index_stride, fd,
                                      fd_stride, attn, negative_slope, grad_logits, grad_fd,
                                      grad_attn, scratch, scratch_bytes, num_heads, num_rows,
                                      num_cols, num_edges, dim_origin, dim_k, stream);
}

extern "C" int maxk_gatv2_score_backward_cols(
    const int32_t* ptr_t, const int32_t* idx_t, const int32_t* order, const float* sp_data,
    int64_t data_stride, const uint8_t* sp_index, int64_t index_stride, const float* fd,
    int64_t fd_stride, const float* attn, float negative_slope, const float* grad_logits,
    float* grad_sp, int32_t num_heads, int32_t num_rows, int32_t num_cols, int64_t num_edges,
    int32_t dim_origin, int32_t dim_k, void* stream) {
  return maxk_v2::score_backward_cols(ptr_t, idx_t, order, sp_data, data_stride, sp_index,
                                      index_stride, fd, fd_stride, attn, negative_slope,
                                      grad_logits, grad_sp, num_heads, num_rows, num_cols,
                                      num_edges, dim_origin, dim_k, stream);
}

extern "C" int maxk_edge_softmax_forward_heads(const int32_t* ptr, const float* logits, float* out,
                                               int32_t num_heads, int32_t num_rows,
                                               int64_t num_edges, void* stream) {
  using namespace maxk_v2;
  const float* ins[1] = {logits};
  bool run;
  const int rc = softmax_check("maxk_edge_softmax_forward_heads: ", ptr, ins, 1, out, num_heads,
                               num_rows, num_edges, run);
  if (!run) return rc;
  dim3 grid = maxk::es_grid(num_rows);
  grid.y = (unsigned)num_heads;
  hipLaunchKernelGGL(edge_softmax_fwd_heads_kernel, grid, dim3(maxk::kEsThreads), 0,
                     (hipStream_t)stream, ptr, logits, out, num_rows, num_edges);
  MAXK_LAUNCH_CHECK("maxk_edge_softmax_forward_heads launch");
  return MAXK_OK;
}

extern "C" int maxk_edge_softmax_backward_heads(const int32_t* ptr, const float* y,
                                                const float* grad_y, float* grad_logits,
                                                int32_t num_heads, int32_t num_rows,
                                                int64_t num_edges, void* stream) {
  using namespace maxk_v2;
  const float* ins[2] = {y, grad_y};
  bool run;
  const int rc = softmax_check("maxk_edge_softmax_backward_heads: ", ptr, ins, 2, grad_logits,
                               num_heads, num_rows, num_edges, run);
  if (!run) return rc;
  dim3 grid = maxk::es_grid(num_rows);
  grid.y = (unsigned)num_heads;
  hipLaunchKernelGGL(edge_softmax_bwd_heads_kernel, grid, dim3(maxk::kEsThreads), 0,
                     (hipStream_t)stream, ptr, y, grad_y, grad_logits, num_rows, num_edges);
  MAXK_LAUNCH_CHECK("maxk_edge_softmax_backward_heads launch");
  return MAXK_OK;
}

extern "C" int64_t maxk_gatv2_scratch_bytes(int32_t num_rows, int32_t dim_origin) {
  return maxk_v2::scratch_bytes(num_rows, dim_origin);
}

extern "C" int maxk_gatv2_row_limits(int32_t* out, int32_t capacity) {
  namespace lg = maxk::lg;
  return maxk::copy_limits(out, capacity,
                           {lg::kShortMax, lg::kMediumMax, lg::kShortMax, lg::kMediumMax});
}
