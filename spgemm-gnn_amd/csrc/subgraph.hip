// Induced subgraphs (include/maxk_hip.h, "Induced subgraphs"): A[nodes][:, nodes] of a square CSR
// graph as a CSR graph over the positions of `nodes`.
//
//   maxk_induced_subgraph_count  out_ptr = the exclusive scan of the kept edges per position,
//                                counts = {M, distinct nodes, entries out of range}
//   maxk_induced_subgraph_fill   out_col / out_eid behind that out_ptr
//
// Both calls first build the local numbering in their scratch: mark[c] = the lowest position that
// names node c (an atomicMin whose result is not read, on an array the call initialised), NONE for
// a node that is not selected. An edge is kept when the mark of its column is not NONE, and that
// mark is its local column. One kernel serves both calls (template argument FILL, the variant
// table's content): a work-group of 4 waves owns a tile of 16 positions and serves each row by its
// length, at most kSgShortMax edges by a lane group of 16, at most kSgMediumMax by one wave, a
// longer one by the whole work-group. A wave reads idx as quads, one aligned 16-byte load per lane
// and chunk of 256 edges, and issues the four mark gathers of every quad of its segment before
// the first of them is used; the gather into the 4 * num_nodes table is the request that bounds
// the kernel. Kept edges are counted and placed by popcounts of ballots below the lane, so the
// order of the edges is the row's and no regime shows in the result.
//
// The exclusive sum over the positions is the shared scan of scan.h; its first two steps also
// count the distinct nodes and the entries out of range (PositionItem).
#include <climits>

#include "common.h"
#include "scan.h"
#include "variants_subgraph.h"

namespace maxk_sg {

using maxk::check_ranges;
using maxk::clampi;
using maxk::Range;
using maxk::set_error;

constexpr int32_t kNone = INT_MAX;  // mark of a node that is not selected

struct SubArgs {
  const int32_t* ptr;
  const int32_t* idx;
  const int32_t* nodes;
  int32_t* out_ptr;
  int32_t* out_col;
  int32_t* out_eid;
  int32_t* counts;
  int32_t* mark;  // int32 [N]: the lowest position that names the node, kNone
  int32_t S, N;
  int64_t E, capacity;
};

// Segment [lo, hi) of the row that position i names, clamped (memory safety; the clamped node is
// the defined one, see the header).
__device__ __forceinline__ void row_segment(const SubArgs& a, int64_t i, int64_t& lo, int64_t& hi) {
  maxk::clamped_segment(a.ptr, a.nodes, i, a.S, a.N, a.E, lo, hi);
}

// The 16-byte boundary of idx at or below edge lo, as an edge number (it may be negative by up
// to 3 when idx itself is not aligned: such quads are read edge by edge).
__device__ __forceinline__ int64_t quad_floor(const int32_t* idx, int64_t lo) {
  const int64_t mis = (int64_t)((reinterpret_cast<uintptr_t>(idx) >> 2) & (kSgQuad - 1));
  return lo - ((lo + mis) & (kSgQuad - 1));
}

// ---------------------------------------------------------------------------------- marks
__global__ __launch_bounds__(kSgThreads) void mark_init_kernel(const SubArgs a) {
  const int64_t c = (int64_t)blockIdx.x * kSgThreads + threadIdx.x;
  if (c < a.N) a.mark[c] = kNone;
}

// The lowest position that names a node: a minimum, so no order of execution shows.
__global__ __launch_bounds__(kSgThreads) void mark_nodes_kernel(const SubArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kSgThreads + threadIdx.x;
  if (i < a.S) atomicMin(a.mark + clampi(a.nodes[i], a.N - 1), (int32_t)i);
}

// ----------------------------------------------------------------------------------- rows
// What one wave holds of CH chunks of a row: the local column of every edge of its quads (kNone:
// not kept, or outside the row), the place of a kept edge among the kept edges of the segment,
// and their number.
template <int CH>
struct Segment {
  int32_t m[CH][kSgQuad];
  int32_t pos[CH][kSgQuad];
  int32_t total;
};

// Lane `lane` of the calling wave takes the quads at start + c * kSgChunk + 4 * lane of the row
// [lo, hi); start is a 16-byte boundary of idx. All loads of idx, then all gathers of marks, then
// the ballots.
template <int CH>
__device__ __forceinline__ void scan_segment(const SubArgs& a, int64_t start, int64_t lo,
                                             int64_t hi, int lane, uint64_t below,
                                             Segment<CH>& s) {
  int32_t col[CH][kSgQuad];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int64_t base = start + (int64_t)c * kSgChunk + (int64_t)kSgQuad * lane;
    const bool any = base < hi && base + kSgQuad > lo;
    if (any && base >= 0 && base + kSgQuad <= a.E) {
      const int4 v = *reinterpret_cast<const int4*>(a.idx + base);
      col[c][0] = v.x;
      col[c][1] = v.y;
      col[c][2] = v.z;
      col[c][3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < kSgQuad; ++j) {
        const int64_t e = base + j;
        col[c][j] = (any && e >= lo && e < hi) ? a.idx[e] : 0;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int64_t base = start + (int64_t)c * kSgChunk + (int64_t)kSgQuad * lane;
#pragma unroll
    for (int j = 0; j < kSgQuad; ++j) {
      const int64_t e = base + j;
      s.m[c][j] = (e >= lo && e < hi) ? a.mark[clampi(col[c][j], a.N - 1)] : kNone;
    }
  }
  int32_t total = 0;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    int32_t under = 0, all = 0;
#pragma unroll
    for (int j = 0; j < kSgQuad; ++j) {
      const uint64_t kept = __ballot(s.m[c][j] != kNone);
      under += __popcll(kept & below);
      all += __popcll(kept);
    }
    int32_t p = total + under;  // kept edges of the lower chunks, of the lower lanes of this one
#pragma unroll
    for (int j = 0; j < kSgQuad; ++j) {
      s.pos[c][j] = p;
      p += (int32_t)(s.m[c][j] != kNone);
    }
    total += all;
  }
  s.total = total;
}

// Kept edge to place `at` of the outputs: nothing is written outside [0, capacity).
__device__ __forceinline__ void emit(const SubArgs& a, int64_t at, int32_t local, int64_t e) {
  if (at >= 0 && at < a.capacity) {
    a.out_col[at] = local;
    a.out_eid[at] = (int32_t)e;
  }
}

template <int CH>
__device__ __forceinline__ void emit_segment(const SubArgs& a, int64_t start, int64_t o, int lane,
                                             const Segment<CH>& s) {
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int64_t base = start + (int64_t)c * kSgChunk + (int64_t)kSgQuad * lane;
#pragma unroll
    for (int j = 0; j < kSgQuad; ++j)
      if (s.m[c][j] != kNone) emit(a, o + s.pos[c][j], s.m[c][j], base + j);
  }
}

// FILL = false: out_ptr[i] = the kept edges of position i for i < S, out_ptr[S] = 0 (the items of
// the scan). FILL = true: out_col / out_eid of position i from out_ptr[i] on.
template <bool FILL>
__global__ __launch_bounds__(kSgThreads) void subgraph_rows_kernel(const SubArgs a) {
  constexpr int G = kSgWave / kSgGroup;  // lane groups of a wave
  static_assert(kSgWaves * G == kSgTile, "one lane group per position of the tile");
  __shared__ int32_t red[kSgWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kSgWave - 1), wave = tid / kSgWave;
  const int g = lane / kSgGroup, sub = lane % kSgGroup, gid = wave * G + g;
  const int64_t i0 = (int64_t)blockIdx.x * kSgTile;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kSgWave - lane));  // lanes under this one
  int64_t lo, hi;

  // short rows: one lane group each, lane `sub` holds edge `sub`; every lane of the wave runs
  // the ballot
  {
    const int64_t i = i0 + gid;
    row_segment(a, i, lo, hi);
    const bool mine = i <= a.S && hi - lo <= kSgShortMax;
    const bool valid = mine && lo + sub < hi;
    const int32_t m = valid ? a.mark[clampi(a.idx[lo + sub], a.N - 1)] : kNone;
    const uint64_t kept = __ballot(m != kNone);
    const uint64_t grp = (kept >> (g * kSgGroup)) & ((1ull << kSgGroup) - 1);
    if constexpr (FILL) {
      if (m != kNone)
        emit(a, (int64_t)a.out_ptr[i] + __popcll(grp & ((1ull << sub) - 1)), m, lo + sub);
    } else {
      if (mine && sub == 0) a.out_ptr[i] = __popcll(grp);
    }
  }

  // medium rows: one wave each (wave-uniform branch)
  for (int t = wave; t < kSgTile; t += kSgWaves) {
    const int64_t i = i0 + t;
    row_segment(a, i, lo, hi);
    if (hi - lo <= kSgShortMax || hi - lo > kSgMediumMax) continue;
    const int64_t start = quad_floor(a.idx, lo);
    Segment<kSgMediumChunks> s;
    scan_segment(a, start, lo, hi, lane, below, s);
    if constexpr (FILL) {
      emit_segment(a, start, (int64_t)a.out_ptr[i], lane, s);
    } else {
      if (lane == 0) a.out_ptr[i] = s.total;
    }
  }

  // hub rows: the whole work-group (block-uniform branch), kSgHubPass edges per pass, a wave on
  // kSgHubChunks consecutive chunks of it
  for (int t = 0; t < kSgTile; ++t) {
    const int64_t i = i0 + t;
    row_segment(a, i, lo, hi);
    if (hi - lo <= kSgMediumMax) continue;
    const int64_t start = quad_floor(a.idx, lo);
    const int64_t o = FILL ? (int64_t)a.out_ptr[i] : 0;
    int32_t base = 0;  // FILL: kept edges of the passes before; else this wave's kept edges
    for (int64_t p0 = start; p0 < hi; p0 += kSgHubPass) {
      const int64_t mine = p0 + (int64_t)wave * kSgHubChunks * kSgChunk;
      Segment<kSgHubChunks> s;
      scan_segment(a, mine, lo, hi, lane, below, s);
      if constexpr (FILL) {
        __syncthreads();  // red is free (the previous pass was read)
        if (lane == 0) red[wave] = s.total;
        __syncthreads();
        int32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kSgWaves; ++w) {
          before += w < wave ? red[w] : 0;
          all += red[w];
        }
        emit_segment(a, mine, o + base + before, lane, s);
        base += all;
      } else {
        base += s.total;
      }
    }
    if constexpr (!FILL) {
      __syncthreads();  // red is free
      if (lane == 0) red[wave] = base;
      __syncthreads();
      if (tid == 0) a.out_ptr[i] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    __syncthreads();  // red changes hands to the next hub row
  }
}

// ---------------------------------------------------------------------------------- scan
// Item i of the scan over the positions 0 .. S: the kept edges of position i, and for i < S
// whether position i is the lowest of its node, and whether its entry lies outside [0, N).
struct PositionItem {
  static constexpr int kSums = 3;
  const int32_t* out_ptr;
  const int32_t* nodes;
  const int32_t* mark;
  int32_t S, N;
  __device__ __forceinline__ void operator()(int64_t i, int32_t (&s)[3]) const {
    s[0] += out_ptr[i];
    if (i < S) {
      const int32_t x = nodes[i];
      s[1] += (int32_t)(mark[clampi(x, N - 1)] == (int32_t)i);
      s[2] += (int32_t)(x < 0 || x >= N);
    }
  }
};

// ------------------------------------------------------------------------------ entry points
static unsigned blocks_of(int64_t n) { return (unsigned)((n + kSgThreads - 1) / kSgThreads); }

// one int32 per node, and three sums per tile of the positions 0 .. S
static int64_t scratch_bytes_of(int64_t N, int64_t S) {
  return 4 * (N + PositionItem::kSums * maxk_scan::tiles(S + 1));
}

static int check_sizes(const std::string& w, int32_t N, int64_t E, int32_t S, int64_t capacity,
                       int64_t scratch_bytes) {
  MAXK_CHECK_ARG(N >= 0 && E >= 0 && E <= (int64_t)INT32_MAX, w + "sizes out of range");
  MAXK_CHECK_ARG(S >= 0, w + "sizes out of range: negative number of selected nodes");
  MAXK_CHECK_ARG(capacity >= 0 && capacity <= (int64_t)INT32_MAX,
                 w + "the bound of out_col / out_eid must fit int32");
  MAXK_CHECK_ARG(S == 0 || N > 0, w + "sizes out of range: nodes selected from an empty graph");
  MAXK_CHECK_ARG(scratch_bytes >= scratch_bytes_of(N, S),
                 w + "scratch_bytes is below maxk_induced_subgraph_scratch_bytes");
  return MAXK_OK;
}

static void launch_marks(const SubArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(mark_init_kernel, dim3(blocks_of(a.N)), dim3(kSgThreads), 0, st, a);
  hipLaunchKernelGGL(mark_nodes_kernel, dim3(blocks_of(a.S)), dim3(kSgThreads), 0, st, a);
}

static int launch_rows(const SubArgs& a, bool fill, hipStream_t st) {
  const int64_t items = (int64_t)a.S + (fill ? 0 : 1);
  const dim3 grid((unsigned)((items + kSgTile - 1) / kSgTile));
  return maxk::dispatch_variant(
      kSubgraphVariants, select_subgraph_variant(fill), [&](auto i) -> int {
        constexpr SubgraphVariant v = kSubgraphVariants[decltype(i)::value];
        hipLaunchKernelGGL(subgraph_rows_kernel<v.fill>, grid, dim3(kSgThreads), 0, st, a);
        return MAXK_OK;
      });
}

static int count_impl(const int32_t* ptr, const int32_t* idx, const int32_t* nodes,
                      int32_t* out_ptr, int32_t* counts, void* scratch, int64_t scratch_bytes,
                      int32_t N, int64_t E, int32_t S, void* stream) {
  const std::string w("maxk_induced_subgraph_count: ");
  if (int rc = check_sizes(w, N, E, S, 0, scratch_bytes)) return rc;
  const int64_t need = scratch_bytes_of(N, S);
  const Range ins[3] = {{ptr, S > 0 ? 4 * ((int64_t)N + 1) : 0},
                        {idx, S > 0 ? 4 * E : 0},
                        {nodes, 4 * (int64_t)S}};
  const Range outs[3] = {{out_ptr, 4 * ((int64_t)S + 1)}, {counts, 12}, {scratch, need}};
  if (int rc = check_ranges(w, ins, 3, outs, 3)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) {
    MAXK_HIP_TRY(hipMemsetAsync(out_ptr, 0, 4, st));
    MAXK_HIP_TRY(hipMemsetAsync(counts, 0, 12, st));
    return MAXK_OK;
  }
  int32_t* mark = static_cast<int32_t*>(scratch);
  const int64_t n = (int64_t)S + 1;
  int32_t* sums = mark + N;  // [3][tiles]: kept edges, first positions, strays
  const SubArgs a{ptr, idx, nodes, out_ptr, nullptr, nullptr, counts, mark, S, N, E, 0};
  launch_marks(a, st);
  if (int e = launch_rows(a, false, st)) return e;
  maxk_scan::launch_tile_sums(PositionItem{out_ptr, nodes, mark, S, N}, n, sums, st);
  maxk_scan::launch_partials<3>(sums, maxk_scan::tiles(n), counts, st);
  maxk_scan::launch_apply(out_ptr, n, sums, st);
  MAXK_LAUNCH_CHECK("maxk_induced_subgraph_count launch");
  return MAXK_OK;
}

static int fill_impl(const int32_t* ptr, const int32_t* idx, const int32_t* nodes,
                     const int32_t* out_ptr, int32_t* out_col, int32_t* out_eid, int64_t capacity,
                     void* scratch, int64_t scratch_bytes, int32_t N, int64_t E, int32_t S,
                     void* stream) {
  const std::string w("maxk_induced_subgraph_fill: ");
  if (int rc = check_sizes(w, N, E, S, capacity, scratch_bytes)) return rc;
  const int64_t need = scratch_bytes_of(N, S);
  const Range ins[4] = {{ptr, S > 0 ? 4 * ((int64_t)N + 1) : 0},
                        {idx, S > 0 ? 4 * E : 0},
                        {nodes, 4 * (int64_t)S},
                        {out_ptr, 4 * ((int64_t)S + 1)}};
  const Range outs[3] = {{out_col, S > 0 ? 4 * capacity : 0},
                         {out_eid, S > 0 ? 4 * capacity : 0},
                         {scratch, need}};
  if (int rc = check_ranges(w, ins, 4, outs, 3)) return rc;
  if (S == 0) return MAXK_OK;
  hipStream_t st = (hipStream_t)stream;
  const SubArgs a{ptr,     idx, nodes, const_cast<int32_t*>(out_ptr),   out_col, out_eid,
                  nullptr, static_cast<int32_t*>(scratch), S, N, E, capacity};
  launch_marks(a, st);
  if (int e = launch_rows(a, true, st)) return e;
  MAXK_LAUNCH_CHECK("maxk_induced_subgraph_fill launch");
  return MAXK_OK;
}

}  // namespace maxk_sg

extern "C" int64_t maxk_induced_subgraph_scratch_bytes(int32_t num_nodes, int32_t num_sel) {
  return (num_nodes < 0 || num_sel < 0) ? 0 : maxk_sg::scratch_bytes_of(num_nodes, num_sel);
}

extern "C" int maxk_induced_subgraph_count(const int32_t* ptr, const int32_t* idx,
                                           const int32_t* nodes, int32_t* out_ptr,
                                           int32_t* counts, void* scratch, int64_t scratch_bytes,
                                           int32_t num_nodes, int64_t num_edges, int32_t num_sel,
                                           void* stream) {
  return maxk_sg::count_impl(ptr, idx, nodes, out_ptr, counts, scratch, scratch_bytes, num_nodes,
                             num_edges, num_sel, stream);
}

extern "C" int maxk_induced_subgraph_fill(const int32_t* ptr, const int32_t* idx,
                                          const int32_t* nodes, const int32_t* out_ptr,
                                          int32_t* out_col, int32_t* out_eid, int64_t capacity,
                                          void* scratch, int64_t scratch_bytes, int32_t num_nodes,
                                          int64_t num_edges, int32_t num_sel, void* stream) {
  return maxk_sg::fill_impl(ptr, idx, nodes, out_ptr, out_col, out_eid, capacity, scratch,
                            scratch_bytes, num_nodes, num_edges, num_sel, stream);
}

extern "C" int maxk_subgraph_row_limits(int32_t* out, int32_t capacity) {
  return maxk::copy_limits(out, capacity, {maxk_sg::kSgShortMax, maxk_sg::kSgMediumMax});
}
