// Neighbour sampling and block compaction (include/maxk_hip.h, "Neighbour sampling").
//
//   maxk_sample_neighbors  per seed row, the `fanout` in-edges of lowest rank
//                              rank(e) = key(e) << 32 | e,  key a counter-based hash of (seed, e)
//                          emitted in ascending edge number; out_ptr is the exclusive scan of
//                          min(row length, fanout)
//   maxk_block_compact     the relabelling of the sampled columns into a compact block: the seeds
//                          first, then every other sampled column once, ascending
//
// The sampler has no global atomics and a fixed result: ranks are unique, so "the fanout lowest"
// is one set whatever order the lanes look at them in. A work-group of 4 waves owns a tile of 16
// seeds and serves each row by its length: at most kSpShortMax edges by a lane group of 16 (every
// lane counts the ranks below its own), at most kSpMediumMax by one wave with the ranks in
// registers, a longer one by the whole work-group, which recomputes the ranks from the hash in
// every pass instead of storing them. The wave and the work-group find the fanout-th lowest rank
// by bisection on its bits from the top (the count of ranks below a candidate is monotone in the
// candidate; the walk stops as soon as a candidate has exactly `fanout` ranks below it, after about
// log2 n + 2 passes), then keep everything at or below it and compact by ballots, which preserves
// the edge order. The position of an edge inside its row replaces the edge number in the rank's low word
// (the same order), so the bisection walks 32 key bits and ceil(log2 n) position bits.
//
// Both entry points need exclusive sums (over the seeds, over the columns): the shared scan of
// scan.h, through caller-supplied scratch whose size an entry point reports. The sampler scans its
// counts as they are; the compaction's tile sums count the new and the seed columns, and its own
// kernel places the new columns behind the scanned sums.
#include <climits>

#include "common.h"
#include "scan.h"
#include "variants_sample.h"

namespace maxk_sp {

using maxk::check_ranges;
using maxk::clampi;
using maxk::Range;
using maxk::set_error;
using maxk_scan::block_exclusive;

__device__ __forceinline__ uint32_t fmix32(uint32_t x) {  // murmur3 finaliser
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

// key(e) of the header: 32 bits from (seed = hi:lo, edge number e)
__device__ __forceinline__ uint32_t edge_key(uint32_t lo, uint32_t hi, uint32_t e) {
  return fmix32(fmix32(e ^ lo) ^ fmix32(e * 0x9E3779B1u + hi));
}

// Segment [b, b + n) of the row that seed position i names, clamped (memory safety, not a
// defined result).
__device__ __forceinline__ void seed_segment(const int32_t* __restrict__ ptr,
                                             const int32_t* __restrict__ seeds, int64_t i,
                                             int32_t S, int32_t num_rows, int64_t E, int64_t& b,
                                             int32_t& n) {
  int64_t e;
  maxk::clamped_segment(ptr, seeds, i, S, num_rows, E, b, e);
  n = (int32_t)(e - b);
}

struct SampleArgs {
  const int32_t* ptr;
  const int32_t* idx;
  const int32_t* seeds;
  int32_t* out_ptr;
  int32_t* out_col;
  int32_t* out_eid;
  int32_t S, num_rows;
  int64_t E, capacity;
  int32_t fanout;
  uint32_t lo, hi;
};

// ------------------------------------------------------------------------------------ counts
// counts of the sampler: out_ptr[i] = min(n_i, fanout) (n_i for fanout < 0), out_ptr[S] = 0
__global__ __launch_bounds__(kSpThreads) void sample_count_kernel(const SampleArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kSpThreads + threadIdx.x;
  if (i > a.S) return;
  int64_t b;
  int32_t n;
  seed_segment(a.ptr, a.seeds, i, a.S, a.num_rows, a.E, b, n);
  a.out_ptr[i] = (a.fanout < 0 || n < a.fanout) ? n : a.fanout;
}

// ----------------------------------------------------------------------------------- sampler
__device__ __forceinline__ uint64_t make_rank(const SampleArgs& a, int64_t b, int32_t j) {
  return ((uint64_t)edge_key(a.lo, a.hi, (uint32_t)(b + j)) << 32) | (uint32_t)j;
}

// Edge j of the row at b to place `pos` of the seed's output segment at o.
__device__ __forceinline__ void emit(const SampleArgs& a, int64_t o, int32_t pos, int64_t b,
                                     int32_t j) {
  const int64_t at = o + pos;
  if (at < a.capacity) {
    a.out_col[at] = a.idx[b + j];
    a.out_eid[at] = (int32_t)(b + j);
  }
}

// bits of the position word that can differ inside a row of n edges
__device__ __forceinline__ int position_bits(int32_t n) { return n > 1 ? 32 - __clz(n - 1) : 0; }

template <bool ALL>
__global__ __launch_bounds__(kSpThreads) void sample_kernel(const SampleArgs a) {
  constexpr int G = kSpWave / kSpGroup;  // lane groups of a wave
  constexpr int NG = kSpWaves * G;       // of the work-group
  static_assert(NG == kSpTile, "one lane group per seed of the tile");
  __shared__ int32_t red[kSpWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kSpWave - 1), wave = tid / kSpWave;
  const int g = lane / kSpGroup, sub = lane % kSpGroup, gid = wave * G + g;
  const int64_t i0 = (int64_t)blockIdx.x * kSpTile;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kSpWave - lane));  // lanes under this one
  int64_t b;
  int32_t n;

  // short rows: one lane group each, lane `sub` holds edge `sub`; every lane of the wave runs
  // the shuffles and the ballot
  {
    const int64_t i = i0 + gid;
    seed_segment(a.ptr, a.seeds, i, a.S, a.num_rows, a.E, b, n);
    const bool mine = i < a.S && n <= kSpShortMax;
    const bool valid = mine && sub < n;
    bool keep = valid;
    if constexpr (!ALL) {
      const uint64_t r = valid ? make_rank(a, b, sub) : ~0ull;
      int32_t under = 0;
#pragma unroll
      for (int m = 0; m < kSpGroup; ++m) {
        const uint32_t olo = __shfl((uint32_t)r, g * kSpGroup + m, kSpWave);
        const uint32_t ohi = __shfl((uint32_t)(r >> 32), g * kSpGroup + m, kSpWave);
        under += (int32_t)((((uint64_t)ohi << 32) | olo) < r);
      }
      keep = valid && (n <= a.fanout || under < a.fanout);
    }
    const uint64_t kept = __ballot(keep);
    if (keep) {
      const uint64_t grp = (kept >> (g * kSpGroup)) & ((1ull << kSpGroup) - 1);
      emit(a, a.out_ptr[i], __popcll(grp & ((1ull << sub) - 1)), b, sub);
    }
  }

  // medium rows: one wave each (wave-uniform branch), edge j in lane j % 64, slot j / 64
  for (int t = wave; t < kSpTile; t += kSpWaves) {
    const int64_t i = i0 + t;
    seed_segment(a.ptr, a.seeds, i, a.S, a.num_rows, a.E, b, n);
    if (n <= kSpShortMax || n > kSpMediumMax) continue;
    const int64_t o = a.out_ptr[i];
    bool keep[kSpSlots];
#pragma unroll
    for (int q = 0; q < kSpSlots; ++q) keep[q] = q * kSpWave + lane < n;
    if constexpr (!ALL) {
      if (n > a.fanout) {
        uint64_t r[kSpSlots];
#pragma unroll
        for (int q = 0; q < kSpSlots; ++q)
          r[q] = keep[q] ? make_rank(a, b, q * kSpWave + lane) : ~0ull;
        uint64_t T = 0;
        const int pb = position_bits(n);
        for (int step = 0; step < 32 + pb; ++step) {
          const int bit = step < 32 ? 63 - step : pb - 1 - (step - 32);
          const uint64_t cand = T | (1ull << bit);
          int32_t c = 0;
#pragma unroll
          for (int q = 0; q < kSpSlots; ++q) c += __popcll(__ballot(r[q] < cand));
          if (c == a.fanout) {  // exactly the fanout lowest lie below cand: done early
            T = cand - 1;
            break;
          }
          if (c < a.fanout) T = cand;
        }
#pragma unroll
        for (int q = 0; q < kSpSlots; ++q) keep[q] = keep[q] && r[q] <= T;
      }
    }
    int32_t base = 0;
#pragma unroll
    for (int q = 0; q < kSpSlots; ++q) {
      const uint64_t kept = __ballot(keep[q]);
      if (keep[q]) emit(a, o, base + __popcll(kept & below), b, q * kSpWave + lane);
      base += __popcll(kept);
    }
  }

  // hub rows: the whole work-group (block-uniform branch); the ranks are recomputed per pass
  for (int t = 0; t < kSpTile; ++t) {
    const int64_t i = i0 + t;
    seed_segment(a.ptr, a.seeds, i, a.S, a.num_rows, a.E, b, n);
    if (n <= kSpMediumMax) continue;
    const int64_t o = a.out_ptr[i];
    uint64_t T = ~0ull;
    if constexpr (!ALL) {
      if (n > a.fanout) {
        T = 0;
        const int pb = position_bits(n);
        for (int step = 0; step < 32 + pb; ++step) {
          const int bit = step < 32 ? 63 - step : pb - 1 - (step - 32);
          const uint64_t cand = T | (1ull << bit);
          int32_t c = 0;
          for (int64_t j0 = 0; j0 < n; j0 += kSpThreads) {
            const int64_t j = j0 + tid;
            c += __popcll(__ballot(j < n && make_rank(a, b, (int32_t)j) < cand));
          }
          __syncthreads();  // red is free (the previous pass was read)
          if (lane == 0) red[wave] = c;
          __syncthreads();
          const int32_t total = (red[0] + red[1]) + (red[2] + red[3]);
          if (total == a.fanout) {  // exactly the fanout lowest lie below cand: done early
            T = cand - 1;
            break;
          }
          if (total < a.fanout) T = cand;
        }
      }
    }
    int32_t base = 0;
    for (int64_t j0 = 0; j0 < n; j0 += kSpThreads) {
      const int64_t j = j0 + tid;
      bool keep = j < n;
      if constexpr (!ALL) keep = keep && (T == ~0ull || make_rank(a, b, (int32_t)j) <= T);
      const uint64_t kept = __ballot(keep);
      __syncthreads();  // red is free
      if (lane == 0) red[wave] = __popcll(kept);
      __syncthreads();
      int32_t before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < kSpWaves; ++w) {
        before += w < wave ? red[w] : 0;
        all += red[w];
      }
      if (keep) emit(a, o, base + before + __popcll(kept & below), b, (int32_t)j);
      base += all;
    }
    __syncthreads();  // red changes hands to the next hub row
  }
}

// -------------------------------------------------------------------------------- compaction
constexpr int32_t kNewColumn = INT_MAX - 1;  // a sampled column that is no seed
constexpr int32_t kNoColumn = INT_MAX;       // a column the block does not hold

// Item c of the compaction's scan: whether column c is a new one, and whether it is a seed.
struct ColumnItem {
  static constexpr int kSums = 2;
  const int32_t* mark;
  __device__ __forceinline__ void operator()(int64_t c, int32_t (&s)[2]) const {
    const int32_t x = mark[c];
    s[0] += (int32_t)(x == kNewColumn);
    s[1] += (int32_t)(x < kNewColumn);
  }
};

struct CompactArgs {
  const int32_t* seeds;
  const int32_t* cols;
  int32_t* src_ids;
  int32_t* local_col;
  int32_t* counts;
  int32_t* mark;  // int32 [num_cols]: the column's place in src_ids, kNewColumn, kNoColumn
  int32_t S, num_cols;
  int64_t M, capacity;
};

// mark[c] = kNoColumn: the entry point initialises its scratch itself
__global__ __launch_bounds__(kSpThreads) void compact_init_kernel(const CompactArgs a) {
  const int64_t c = (int64_t)blockIdx.x * kSpThreads + threadIdx.x;
  if (c < a.num_cols) a.mark[c] = kNoColumn;
}

// Seeds: the lowest position that names a column (a minimum, so no order of execution shows);
// sampled columns: kNewColumn unless a seed. Neither atomic returns a value.
__global__ __launch_bounds__(kSpThreads) void compact_mark_kernel(const CompactArgs a, int what) {
  const int64_t i = (int64_t)blockIdx.x * kSpThreads + threadIdx.x;
  if (what == 0) {
    if (i >= a.S) return;
    const int32_t s = a.seeds[i];
    if (i < a.capacity) a.src_ids[i] = s;
    atomicMin(a.mark + clampi(s, a.num_cols - 1), (int32_t)i);
  } else {
    if (i >= a.M) return;
    atomicMin(a.mark + clampi(a.cols[i], a.num_cols - 1), kNewColumn);
  }
}

// The new columns in ascending order behind the seeds; counts = {num_src, distinct_seeds}. A
// thread owns the items of the scan's apply step: sums are the scanned tile sums of the new
// columns, totals = {new columns, seed columns}.
__global__ __launch_bounds__(kSpThreads) void compact_place_kernel(const CompactArgs a,
                                                                   const int32_t* sums,
                                                                   const int32_t* totals) {
  constexpr int kItems = maxk_scan::kItems;
  static_assert(kSpThreads == maxk_scan::kThreads, "a work-group of the scan's shape");
  __shared__ int32_t red[maxk_scan::kWaves];
  const int64_t first = (int64_t)blockIdx.x * maxk_scan::kTile + (int64_t)threadIdx.x * kItems;
  bool fresh[kItems];
  int32_t s = 0;
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    fresh[q] = first + q < a.num_cols && a.mark[first + q] == kNewColumn;
    s += (int32_t)fresh[q];
  }
  int32_t total;
  int64_t run = (int64_t)a.S + sums[blockIdx.x] + block_exclusive(s, red, total);
#pragma unroll
  for (int q = 0; q < kItems; ++q) {
    if (!fresh[q]) continue;
    a.mark[first + q] = (int32_t)run;
    if (run < a.capacity) a.src_ids[run] = (int32_t)(first + q);
    ++run;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.counts[0] = a.S + totals[0];
    a.counts[1] = totals[1];
  }
}

__global__ __launch_bounds__(kSpThreads) void compact_relabel_kernel(const CompactArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kSpThreads + threadIdx.x;
  if (i < a.M) a.local_col[i] = a.mark[clampi(a.cols[i], a.num_cols - 1)];
}

// ------------------------------------------------------------------------------ entry points
static unsigned blocks_of(int64_t n) { return (unsigned)((n + kSpThreads - 1) / kSpThreads); }

// partial sums of the tiles (two arrays) and the totals pair, in int32 words
static int64_t scan_words(int64_t n) { return 2 * maxk_scan::tiles(n) + 2; }

static int sample_impl(const int32_t* ptr, const int32_t* idx, const int32_t* seeds,
                       int32_t* out_ptr, int32_t* out_col, int32_t* out_eid, int64_t capacity,
                       void* scratch, int64_t scratch_bytes, int32_t num_rows, int64_t E,
                       int32_t S, int32_t fanout, uint64_t seed, void* stream) {
  const std::string w("maxk_sample_neighbors: ");
  MAXK_CHECK_ARG(num_rows >= 0 && E >= 0 && E <= (int64_t)INT32_MAX, w + "sizes out of range");
  MAXK_CHECK_ARG(S >= 0, w + "sizes out of range: negative number of seeds");
  MAXK_CHECK_ARG(fanout != 0, w + "fanout must be positive, or negative for every neighbour");
  MAXK_CHECK_ARG(capacity >= 0 && capacity <= (int64_t)INT32_MAX,
                 w + "the bound of out_col / out_eid must fit int32");
  MAXK_CHECK_ARG(S == 0 || num_rows > 0, w + "sizes out of range: seeds without rows");
  const int64_t need = 4 * scan_words((int64_t)S + 1);
  MAXK_CHECK_ARG(scratch_bytes >= need, w + "scratch_bytes is below maxk_sample_scratch_bytes");
  const Range ins[3] = {{ptr, S > 0 ? 4 * ((int64_t)num_rows + 1) : 0},
                        {idx, S > 0 ? 4 * E : 0},
                        {seeds, 4 * (int64_t)S}};
  const Range outs[4] = {{out_ptr, 4 * ((int64_t)S + 1)},
                         {out_col, S > 0 ? 4 * capacity : 0},
                         {out_eid, S > 0 ? 4 * capacity : 0},
                         {scratch, need}};
  if (int rc = check_ranges(w, ins, 3, outs, 4)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (S == 0) {
    MAXK_HIP_TRY(hipMemsetAsync(out_ptr, 0, 4, st));
    return MAXK_OK;
  }
  const SampleArgs a{ptr, idx, seeds, out_ptr, out_col, out_eid, S, num_rows, E, capacity,
                     fanout, (uint32_t)seed, (uint32_t)(seed >> 32)};
  const int64_t n = (int64_t)S + 1;
  hipLaunchKernelGGL(sample_count_kernel, dim3(blocks_of(n)), dim3(kSpThreads), 0, st, a);
  maxk_scan::exclusive_scan(out_ptr, n, static_cast<int32_t*>(scratch), st);
  const dim3 grid((unsigned)(((int64_t)S + kSpTile - 1) / kSpTile));
  if (int e = maxk::dispatch_variant(
          kSampleVariants, select_sample_variant(fanout), [&](auto i) -> int {
            constexpr SampleVariant v = kSampleVariants[decltype(i)::value];
            hipLaunchKernelGGL(sample_kernel<v.all>, grid, dim3(kSpThreads), 0, st, a);
            return MAXK_OK;
          }))
    return e;
  MAXK_LAUNCH_CHECK("maxk_sample_neighbors launch");
  return MAXK_OK;
}

static int64_t compact_scratch_bytes(int64_t num_cols) {
  return 4 * (num_cols + scan_words(num_cols));
}

static int compact_impl(const int32_t* seeds, const int32_t* cols, int32_t* src_ids,
                        int64_t capacity, int32_t* local_col, int32_t* counts, void* scratch,
                        int64_t scratch_bytes, int32_t S, int64_t M, int32_t num_cols,
                        void* stream) {
  const std::string w("maxk_block_compact: ");
  MAXK_CHECK_ARG(S >= 0 && num_cols >= 0 && M >= 0 && M <= (int64_t)INT32_MAX,
                 w + "sizes out of range");
  MAXK_CHECK_ARG(capacity >= 0 && capacity <= (int64_t)INT32_MAX,
                 w + "the bound of src_ids must fit int32");
  MAXK_CHECK_ARG((S == 0 && M == 0) || num_cols > 0,
                 w + "sizes out of range: seeds or edges without columns");
  MAXK_CHECK_ARG(capacity >= S, w + "src_ids must hold the seeds");
  const int64_t need = compact_scratch_bytes(num_cols);
  MAXK_CHECK_ARG(scratch_bytes >= need,
                 w + "scratch_bytes is below maxk_block_compact_scratch_bytes");
  const Range ins[2] = {{seeds, 4 * (int64_t)S}, {cols, 4 * M}};
  const Range outs[4] = {{src_ids, 4 * capacity}, {local_col, 4 * M}, {counts, 8},
                         {scratch, need}};
  if (int rc = check_ranges(w, ins, 2, outs, 4)) return rc;
  hipStream_t st = (hipStream_t)stream;
  int32_t* mark = static_cast<int32_t*>(scratch);
  const int64_t nb = maxk_scan::tiles(num_cols);
  int32_t* sums = mark + num_cols;  // [2][nb]: new columns, seed columns
  int32_t* totals = sums + 2 * nb;
  const CompactArgs a{seeds, cols, src_ids, local_col, counts, mark, S, num_cols, M, capacity};
  if (num_cols == 0) {  // no seeds and no edges: {0, 0}
    MAXK_HIP_TRY(hipMemsetAsync(counts, 0, 8, st));
    return MAXK_OK;
  }
  hipLaunchKernelGGL(compact_init_kernel, dim3(blocks_of(num_cols)), dim3(kSpThreads), 0, st, a);
  if (S > 0)
    hipLaunchKernelGGL(compact_mark_kernel, dim3(blocks_of(S)), dim3(kSpThreads), 0, st, a, 0);
  if (M > 0)
    hipLaunchKernelGGL(compact_mark_kernel, dim3(blocks_of(M)), dim3(kSpThreads), 0, st, a, 1);
  maxk_scan::launch_tile_sums(ColumnItem{mark}, (int64_t)num_cols, sums, st);
  maxk_scan::launch_partials<2>(sums, nb, totals, st);
  hipLaunchKernelGGL(compact_place_kernel, dim3((unsigned)nb), dim3(kSpThreads), 0, st, a,
                     (const int32_t*)sums, (const int32_t*)totals);
  if (M > 0)
    hipLaunchKernelGGL(compact_relabel_kernel, dim3(blocks_of(M)), dim3(kSpThreads), 0, st, a);
  MAXK_LAUNCH_CHECK("maxk_block_compact launch");
  return MAXK_OK;
}

}  // namespace maxk_sp

extern "C" int64_t maxk_sample_scratch_bytes(int32_t num_seeds) {
  return num_seeds < 0 ? 0 : 4 * maxk_sp::scan_words((int64_t)num_seeds + 1);
}

extern "C" int maxk_sample_neighbors(const int32_t* ptr, const int32_t* idx, const int32_t* seeds,
                                     int32_t* out_ptr, int32_t* out_col, int32_t* out_eid,
                                     int64_t capacity, void* scratch, int64_t scratch_bytes,
                                     int32_t num_rows, int64_t num_edges, int32_t num_seeds,
                                     int32_t fanout, uint64_t seed, void* stream) {
  return maxk_sp::sample_impl(ptr, idx, seeds, out_ptr, out_col, out_eid, capacity, scratch,
                              scratch_bytes, num_rows, num_edges, num_seeds, fanout, seed, stream);
}

extern "C" int maxk_sample_row_limits(int32_t* out, int32_t capacity) {
  return maxk::copy_limits(out, capacity, {maxk_sp::kSpShortMax, maxk_sp::kSpMediumMax});
}

extern "C" int64_t maxk_block_compact_scratch_bytes(int32_t num_cols) {
  return num_cols < 0 ? 0 : maxk_sp::compact_scratch_bytes(num_cols);
}

extern "C" int maxk_block_compact(const int32_t* seeds, const int32_t* cols, int32_t* src_ids,
                                  int64_t capacity, int32_t* local_col, int32_t* counts,
                                  void* scratch, int64_t scratch_bytes, int32_t num_seeds,
                                  int64_t num_edges, int32_t num_cols, void* stream) {
  return maxk_sp::compact_impl(seeds, cols, src_ids, capacity, local_col, counts, scratch,
                               scratch_bytes, num_seeds, num_edges, num_cols, stream);
}
