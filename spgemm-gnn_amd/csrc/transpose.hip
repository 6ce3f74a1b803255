// CSR transposition (include/maxk_hip.h, "CSR transposition"): A^T of a CSR graph as the stable
// sort of its edges by column, a least-significant-digit radix sort on the column number with
// digits of up to kTrMaxDigitBits bits (variants_transpose.h holds the digit plan).
//
// Per pass, with the items in the order the pass before left them (pass 0: the CSR order):
//
//   zero_kernel          (once) out_ptr = 0
//   tile_hist_kernel     a work-group owns a tile of kTrTile consecutive items, independent of the
//                        rows, and writes its digit counts digit-major, hist[digit][tile]; pass 0
//                        also counts the columns into out_ptr (integer atomics whose results are
//                        not read; their sums are read after a launch boundary)
//   scan (3 launches)    hist becomes its exclusive scan (scan.h): the place of the first item
//                        of digit d of tile t in the pass's output
//   scatter_pass_kernel  wave w of a tile owns the sub-run w of kTrSubRun consecutive items. The
//                        waves count their sub-runs' digits again (LDS atomics, sums only), the
//                        counts of the waves below and the tile's scanned base give each wave a
//                        running base per digit in LDS, and the wave walks its sub-run 64 items
//                        at a time: lanes of equal digit are found by one ballot per digit bit
//                        and ranked by the popcount of their peers below the lane, on top of the
//                        running base. The order inside a digit is the input order by
//                        construction, and no placement reads the result of an atomic.
//
// The first pass reads idx (the edge number is the position), the last pass writes out_order,
// out_row (the row of an edge is found in ptr by bisection) and out_val. Two passes go through one
// (column, edge) buffer in scratch; with three, the first writes its pairs into out_row /
// out_order, the second moves them into scratch and the third writes the outputs. out_ptr is the
// exclusive scan of the column counts of pass 0.
#include <climits>

#include "common.h"
#include "scan.h"
#include "variants_transpose.h"

namespace maxk_tr {

using maxk::check_ranges;
using maxk::clampi;
using maxk::Range;
using maxk::set_error;

struct TrArgs {
  const int32_t* ptr;
  const int32_t* idx;
  const float* val;
  int32_t* out_ptr;
  int32_t* out_row;
  int32_t* out_order;
  float* out_val;
  const int32_t* src_key;  // the pairs a middle / last pass reads
  const int32_t* src_eid;
  int32_t* dst_key;        // the pairs a first / middle pass writes
  int32_t* dst_eid;
  int32_t* hist;           // [1 << bits][tiles]
  int32_t N, NC;
  int64_t E, tiles;
  int32_t shift, bits;     // this pass's digit: (key >> shift) & ((1 << bits) - 1)
};

template <bool FROM_IDX>
__device__ __forceinline__ int32_t load_key(const TrArgs& a, int64_t i) {
  if constexpr (FROM_IDX) {
    return clampi(a.idx[i], a.NC - 1);
  } else {
    return a.src_key[i];
  }
}

// The row r with ptr[r] <= e < ptr[r + 1]: the last row that starts at or before e. Stays inside
// [0, N) whatever ptr holds.
__device__ __forceinline__ int32_t row_of(const TrArgs& a, int32_t e) {
  int32_t lo = 0, hi = a.N - 1;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo + 1) >> 1);
    if (a.ptr[mid] <= e) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  return lo;
}

// cnt[w][d] = 0 for the digits of this pass (whole work-group; a barrier follows at the caller).
__device__ __forceinline__ void zero_counts(int32_t (*cnt)[kTrMaxDigits], int nd) {
  for (int d = threadIdx.x; d < nd; d += kTrThreads) {
#pragma unroll
    for (int w = 0; w < kTrWaves; ++w) cnt[w][d] = 0;
  }
}

// The calling wave adds the digits of its sub-run [first, first + kTrSubRun) to `mine`; COLS: and
// the columns to out_ptr. Sums only: no result of an atomic is read.
template <bool FROM_IDX, bool COLS>
__device__ __forceinline__ void count_sub_run(const TrArgs& a, int32_t* mine, int64_t first,
                                              int lane) {
  const int32_t mask = (1 << a.bits) - 1;
  for (int r = 0; r < kTrRounds; ++r) {
    const int64_t i0 = first + (int64_t)r * kTrWave;
    if (i0 >= a.E) break;
    const int64_t i = i0 + lane;
    if (i < a.E) {
      const int32_t key = load_key<FROM_IDX>(a, i);
      atomicAdd(mine + ((key >> a.shift) & mask), 1);
      if constexpr (COLS) atomicAdd(a.out_ptr + key, 1);
    }
  }
}

template <bool FROM_IDX>
__global__ __launch_bounds__(kTrThreads) void tile_hist_kernel(const TrArgs a) {
  __shared__ int32_t cnt[kTrWaves][kTrMaxDigits];
  const int tid = threadIdx.x, lane = tid & (kTrWave - 1), wave = tid / kTrWave;
  const int nd = 1 << a.bits;
  zero_counts(cnt, nd);
  __syncthreads();
  count_sub_run<FROM_IDX, FROM_IDX>(
      a, cnt[wave], (int64_t)blockIdx.x * kTrTile + (int64_t)wave * kTrSubRun, lane);
  __syncthreads();
  for (int d = tid; d < nd; d += kTrThreads)
    a.hist[(int64_t)d * a.tiles + blockIdx.x] = (cnt[0][d] + cnt[1][d]) + (cnt[2][d] + cnt[3][d]);
}
static_assert(kTrWaves == 4, "the sums above name four waves");

template <int ROLE, bool VAL>
__global__ __launch_bounds__(kTrThreads) void scatter_pass_kernel(const TrArgs a) {
  constexpr bool FROM_IDX = ROLE == kTrFirst || ROLE == kTrOnly;
  constexpr bool FINAL = ROLE == kTrLast || ROLE == kTrOnly;
  static_assert(FINAL || !VAL, "only a pass that writes the outputs gathers values");
  __shared__ int32_t cnt[kTrWaves][kTrMaxDigits];
  const int tid = threadIdx.x, lane = tid & (kTrWave - 1), wave = tid / kTrWave;
  const int nd = 1 << a.bits;
  const int32_t mask = nd - 1;
  const int64_t first = (int64_t)blockIdx.x * kTrTile + (int64_t)wave * kTrSubRun;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (kTrWave - lane));  // lanes under this one

  zero_counts(cnt, nd);
  __syncthreads();
  count_sub_run<FROM_IDX, false>(a, cnt[wave], first, lane);
  __syncthreads();
  // cnt[w][d] becomes where wave w's first item of digit d goes: the tile's scanned base, then
  // the items of the waves below
  for (int d = tid; d < nd; d += kTrThreads) {
    int32_t run = a.hist[(int64_t)d * a.tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kTrWaves; ++w) {
      const int32_t t = cnt[w][d];
      cnt[w][d] = run;
      run += t;
    }
  }
  __syncthreads();

  // every access below is one LDS instruction of this wave, in program order
  volatile int32_t* mine = cnt[wave];
  for (int r = 0; r < kTrRounds; ++r) {
    const int64_t i0 = first + (int64_t)r * kTrWave;
    if (i0 >= a.E) break;  // wave-uniform
    const int64_t i = i0 + lane;
    const bool valid = i < a.E;
    const int32_t key = valid ? load_key<FROM_IDX>(a, i) : 0;
    int32_t eid = (int32_t)i;
    if constexpr (!FROM_IDX) eid = valid ? a.src_eid[i] : 0;
    const int32_t d = (key >> a.shift) & mask;
    uint64_t peers = __ballot(valid);  // the valid lanes with this lane's digit
    for (int b = 0; b < a.bits; ++b) {
      const bool bit = (d >> b) & 1;
      const uint64_t set = __ballot(bit);
      peers &= bit ? set : ~set;
    }
    const int32_t rank = __popcll(peers & below), all = __popcll(peers);
    if (valid) {
      const int32_t base = mine[d];
      if (rank == all - 1) mine[d] = base + all;  // one lane per digit, after every peer's read
      const int32_t pos = base + rank;
      if (pos >= 0 && (int64_t)pos < a.E) {
        if constexpr (FINAL) {
          a.out_order[pos] = eid;
          a.out_row[pos] = row_of(a, eid);
          if constexpr (VAL) {
            const uint32_t* bits = reinterpret_cast<const uint32_t*>(a.val);
            const int64_t e = eid < 0 ? 0 : ((int64_t)eid < a.E ? eid : a.E - 1);
            reinterpret_cast<uint32_t*>(a.out_val)[pos] = bits[e];
          }
        } else {
          a.dst_key[pos] = key;
          a.dst_eid[pos] = eid;
        }
      }
    }
  }
}

// out_ptr before the column counts. A kernel of the library's own and not a memset: the fill of a
// captured memset node was seen to change between replays of one graph.
__global__ __launch_bounds__(kTrThreads) void zero_kernel(int32_t* v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kTrThreads + threadIdx.x;
  if (i < n) v[i] = 0;
}

// ------------------------------------------------------------------------------ entry points
static int64_t tiles_of(int64_t E) { return (E + kTrTile - 1) / kTrTile; }

// The (column, edge) buffer of a sort of more than one pass, the tile histograms of the widest
// digit (the lowest), and one sum per scan tile of the longer of the two scanned arrays.
static int64_t scratch_bytes_of(int64_t NC, int64_t E) {
  if (E == 0) return 0;
  const int32_t nc = (int32_t)NC;
  const int64_t pairs = pass_count(nc) > 1 ? 8 * E : 0;
  const int64_t hist = tiles_of(E) << digit_bits(nc, 0);
  const int64_t longest = hist > NC + 1 ? hist : NC + 1;
  return pairs + 4 * (hist + maxk_scan::tiles(longest));
}

static int transpose_impl(const int32_t* ptr, const int32_t* idx, const float* val,
                          int32_t* out_ptr, int32_t* out_row, int32_t* out_order, float* out_val,
                          void* scratch, int64_t scratch_bytes, int32_t N, int32_t NC, int64_t E,
                          void* stream) {
  const std::string w("maxk_csr_transpose: ");
  MAXK_CHECK_ARG(N >= 0 && NC >= 0 && E >= 0, w + "sizes out of range");
  if (E > (int64_t)INT32_MAX) {
    set_error(w + "num_edges must be below 2^31 (int32 edge numbers)");
    return MAXK_ERR_UNSUPPORTED;
  }
  MAXK_CHECK_ARG(E == 0 || (N > 0 && NC > 0),
                 w + "sizes out of range: edges in a graph without rows or without columns");
  MAXK_CHECK_ARG((val == nullptr) == (out_val == nullptr),
                 w + "val and out_val must both be given or both be NULL");
  const int64_t need = scratch_bytes_of(NC, E);
  MAXK_CHECK_ARG(scratch_bytes >= need,
                 w + "scratch_bytes is below maxk_csr_transpose_scratch_bytes");
  // val / out_val are optional: a NULL one has no bytes
  const Range ins[3] = {{ptr, E > 0 ? 4 * ((int64_t)N + 1) : 0}, {idx, 4 * E},
                        {val, val ? 4 * E : 0}};
  const Range outs[5] = {{out_ptr, 4 * ((int64_t)NC + 1)}, {out_row, 4 * E}, {out_order, 4 * E},
                         {out_val, out_val ? 4 * E : 0},   {scratch, need}};
  if (int rc = check_ranges(w, ins, 3, outs, 5)) return rc;

  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(zero_kernel, dim3((unsigned)(((int64_t)NC + kTrThreads) / kTrThreads)),
                     dim3(kTrThreads), 0, st, out_ptr, (int64_t)NC + 1);
  if (E == 0) {
    MAXK_LAUNCH_CHECK("maxk_csr_transpose launch");
    return MAXK_OK;
  }

  const int passes = pass_count(NC);
  const int64_t tiles = tiles_of(E);
  int32_t* words = static_cast<int32_t*>(scratch);
  int32_t* key_a = words;  // the scratch pair buffer (more than one pass)
  int32_t* eid_a = words + E;
  int32_t* hist = words + (passes > 1 ? 2 * E : 0);
  int32_t* sums = hist + (tiles << digit_bits(NC, 0));
  TrArgs a{ptr, idx, val, out_ptr, out_row, out_order, out_val, nullptr, nullptr, nullptr,
           nullptr, hist, N, NC, E, tiles, 0, 0};
  const dim3 grid((unsigned)tiles), block(kTrThreads);
  for (int pass = 0; pass < passes; ++pass) {
    a.bits = digit_bits(NC, pass);
    a.shift = digit_shift(NC, pass);
    // two passes: idx -> scratch -> outputs; three: idx -> (out_row, out_order) -> scratch ->
    // outputs, so the pass that writes the outputs never reads them
    const bool to_outputs = passes == 3 && pass == 0;
    const bool from_outputs = passes == 3 && pass == 1;
    a.src_key = pass == 0 ? nullptr : (from_outputs ? out_row : key_a);
    a.src_eid = pass == 0 ? nullptr : (from_outputs ? out_order : eid_a);
    a.dst_key = pass == passes - 1 ? nullptr : (to_outputs ? out_row : key_a);
    a.dst_eid = pass == passes - 1 ? nullptr : (to_outputs ? out_order : eid_a);
    if (int e = maxk::dispatch_variant(
            kHistVariants, select_hist_variant(pass), [&](auto i) -> int {
              constexpr HistVariant v = kHistVariants[decltype(i)::value];
              hipLaunchKernelGGL(tile_hist_kernel<v.from_idx>, grid, block, 0, st, a);
              return MAXK_OK;
            }))
      return e;
    maxk_scan::exclusive_scan(hist, tiles << a.bits, sums, st);
    if (int e = maxk::dispatch_variant(
            kPassVariants, select_pass_variant(pass, passes, val != nullptr),
            [&](auto i) -> int {
              constexpr PassVariant v = kPassVariants[decltype(i)::value];
              hipLaunchKernelGGL((scatter_pass_kernel<v.role, v.val>), grid, block, 0, st, a);
              return MAXK_OK;
            }))
      return e;
  }
  maxk_scan::exclusive_scan(out_ptr, (int64_t)NC + 1, sums, st);
  MAXK_LAUNCH_CHECK("maxk_csr_transpose launch");
  return MAXK_OK;
}

}  // namespace maxk_tr

extern "C" int64_t maxk_csr_transpose_scratch_bytes(int32_t num_rows, int32_t num_cols,
                                                    int64_t num_edges) {
  if (num_rows < 0 || num_cols < 0 || num_edges < 0 || num_edges > (int64_t)INT32_MAX) return 0;
  return maxk_tr::scratch_bytes_of(num_cols, num_edges);
}

extern "C" int maxk_csr_transpose(const int32_t* ptr, const int32_t* idx, const float* val,
                                  int32_t* out_ptr, int32_t* out_row, int32_t* out_order,
                                  float* out_val, void* scratch, int64_t scratch_bytes,
                                  int32_t num_rows, int32_t num_cols, int64_t num_edges,
                                  void* stream) {
  return maxk_tr::transpose_impl(ptr, idx, val, out_ptr, out_row, out_order, out_val, scratch,
                                 scratch_bytes, num_rows, num_cols, num_edges, stream);
}

extern "C" int maxk_transpose_digit_bits(int32_t num_cols, int32_t* out, int32_t capacity) {
  const int count = maxk_tr::pass_count(num_cols);
  for (int i = 0; i < count && out && i < capacity; ++i)
    out[i] = maxk_tr::digit_bits(num_cols, i);
  return count;
}
