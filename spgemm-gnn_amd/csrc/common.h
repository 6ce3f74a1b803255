// Shared helpers for the gfx950 MaxK kernels and the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "device_buf.h"
#include "maxk_hip.h"
#include "variants.h"

namespace maxk {

constexpr int kFwdTileRows = 32;        // default destination rows per forward work-group
constexpr int kFwdMaxTileRows = 64;
// forward LDS accumulator row stride D + kFwdRowPad elements: rows start on different banks,
// so lanes of different edges with nearby selectors (sorted CBSR slots) spread over banks
// (Reddit: k = 16 1.354 -> 1.341 ms, k = 32 2.500 -> 2.470, k = 8 0.898 -> 0.905)
constexpr int kFwdRowPad = 1;
// forward edge word: source column in the low kFwdColBits bits, row within the tile above
constexpr int kFwdColBits = 26;
constexpr uint32_t kFwdColMask = (1u << kFwdColBits) - 1;
constexpr int kBwdThreads = 512;        // 8 waves per backward work-group (12 at k >= 32)
constexpr int kMaxDim = 256;            // u8 selectors => D <= 256
constexpr int kBwdTasksPerCu = 2;
constexpr int kBwdMinTaskEdges = 100000;  // a chunk's flush (C*k stores) vs its edges
constexpr int kXcds = 8;
constexpr int kFwdRotWindows = 16;         // column windows of the rotated forward sweep
constexpr double kFwdSlotEdgeRate = 1.6e8;  // edges/s one forward slot sustains at k = 16
constexpr double kFwdSlotEdgeRateFixed = 3.0e8;  // the same with the fixed-point update
// (round 4: 2.6e8 -> 3.0e8 with the 1.5 x task cap, Reddit k = 16 / 32 / 64 -1.0 / -0.2 / -0.3 %;
// 3.5e8 and above slower, profiles/r04/fwd_rot_rate_ab.jsonl)
// CBSR tables (5k bytes per column) above these sizes get packed one-line forward records
// even where two tables would otherwise be used (plan.hip: k >= 32 / k < 32)
constexpr double kFwdPackedTableBytes = 150e6;
constexpr double kFwdPackedTableBytes16 = 32e6;
// k < 32: below kFwdPackMinEdgesPerCol edges per column the forward gathers from the two API
// tables instead of packing one record per column per call; below kFwdPackMinEdgesPerColL2
// too while the selector table (k bytes per column) stays L2-resident, where the second
// (selector) touch of an edge is cheap (plan.hip)
constexpr long long kFwdPackMinEdgesPerCol = 40;
constexpr long long kFwdPackMinEdgesPerColL2 = 128;
constexpr double kFwdSelL2Bytes = 3e6;
// two-pass backward below this many expected edges per (row, column block), i.e. when a
// column block sees each grad_out row it fetches about once. Measured (blocks vs two-pass,
// ms): ogbn-products k = 16 (0.04) 13.4 / 6.0, k = 32 (0.02) 16.0 / 8.3; yelp k = 64 (0.015)
// 1.98 / 1.81; flickr k = 8 (0.50) 0.25 / 0.06; Reddit k = 64 (0.96) 4.86 / 15.2, k = 16 (3.8)
// 1.70 / 5.35; ogbn-proteins k = 8 (15) 0.94 / 2.68
constexpr double kBwdTwoPassReuse = 0.75;
constexpr int kBwdRowsPerWave = 4;  // row pass: most destination rows one wavefront stages
// two-pass backward: the E x k product workspace is cut into row chunks of at most this many
// bytes (one row pass + one column pass per chunk; bwd_tp_chunks overrides)
// (ogbn-products k = 32, 15.8 GB in one chunk: 1 / 2 / 4 / 8 chunks ran 8.11 / 8.68 / 10.49 /
// 14.60 ms; every chunk's column pass visits every column)
constexpr double kBwdTwoPassWorkspaceCap = 16.0 * (1ull << 30);
// work-groups per CU of the fused CBSR pack + statistics pass (each adds one atomic per
// statistics word, and same-address atomics serialise at the L2). Reddit, pack+stats at
// k = 16 / stats at k = 32, 64: 1 -> 24.5 / 54.5 us, 4 -> 20.8 / 26.6 us, 8 -> 31.5 / 33.7 us
// (the separate pack + stats passes took 21 + 17 us at k = 16)
constexpr int kStatsBlocksPerCu = 4;
// Records past the end of the backward edge list that a wave may read (and ignore): one
// iteration of a wave covers at most 16 sub-steps x 64 edges.
constexpr int kBwdRecPad = 16 * kWave + kWave;
constexpr int kBwdLdsBudget = 160 * 1024; // all of a CU's LDS: one work-group per CU

// Thread-local error message plumbing for maxk_last_error().
void set_error(const std::string& msg);

#define MAXK_CHECK_ARG(cond, msg)                 \
  do {                                            \
    if (!(cond)) {                                \
      ::maxk::set_error(msg);                     \
      return MAXK_ERR_INVALID_ARG;                \
    }                                             \
  } while (0)

#define MAXK_HIP_TRY(expr)                                                      \
  do {                                                                          \
    hipError_t _e = (expr);                                                     \
    if (_e != hipSuccess) {                                                     \
      ::maxk::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));     \
      return (int)_e;                                                           \
    }                                                                           \
  } while (0)

#define MAXK_LAUNCH_CHECK(what)                                                 \
  do {                                                                          \
    hipError_t _e = hipGetLastError();                                          \
    if (_e != hipSuccess) {                                                     \
      ::maxk::set_error(std::string(what) + ": " + hipGetErrorString(_e));      \
      return (int)_e;                                                           \
    }                                                                           \
  } while (0)

// Runs fn(std::integral_constant<size_t, I>) for the entry I of `table` that equals `v` and
// returns its result: the launchers name kernel<table[I]...> there, so a family's instantiations
// are its table's entries. A variant outside the table is an error, not a fallback.
template <class Table, class V, class Fn, size_t... I>
int dispatch_variant(const Table& table, const V& v, Fn&& fn, std::index_sequence<I...>) {
  int rc = MAXK_ERR_UNSUPPORTED;
  const bool found =
      ((table[I] == v ? (rc = fn(std::integral_constant<size_t, I>{}), true) : false) || ...);
  if (!found) set_error("no compiled kernel " + kernel_name(v));
  return rc;
}
template <class Table, class V, class Fn>
int dispatch_variant(const Table& table, const V& v, Fn&& fn) {
  return dispatch_variant(table, v, fn, std::make_index_sequence<std::tuple_size<Table>::value>{});
}

// Whether [a, a + na) and [b, b + nb) (bytes) share a byte.
inline bool ranges_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return na > 0 && nb > 0 && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// An array argument of an entry point; an optional one that is absent has no bytes.
struct Range {
  const void* p;
  int64_t bytes;
};

// Refuses a null pointer with bytes, and an output that shares a byte with an input or with
// another output. w: the entry point's name and ": ".
inline int check_ranges(const std::string& w, const Range* ins, int nin, const Range* outs,
                        int nout) {
  bool null = false;
  for (int i = 0; i < nin; ++i) null = null || (ins[i].bytes > 0 && !ins[i].p);
  for (int i = 0; i < nout; ++i) null = null || (outs[i].bytes > 0 && !outs[i].p);
  MAXK_CHECK_ARG(!null, w + "null pointer");
  bool overlap = false;
  for (int o = 0; o < nout; ++o) {
    for (int i = 0; i < nin; ++i)
      overlap = overlap || ranges_overlap(outs[o].p, outs[o].bytes, ins[i].p, ins[i].bytes);
    for (int i = o + 1; i < nout; ++i)
      overlap = overlap || ranges_overlap(outs[o].p, outs[o].bytes, outs[i].p, outs[i].bytes);
  }
  MAXK_CHECK_ARG(!overlap, w + "an output overlaps an input or another output");
  return MAXK_OK;
}

// The body of a maxk_*_row_limits export: the first min(count, capacity) limits into out (NULL:
// none), and the count.
inline int copy_limits(int32_t* out, int32_t capacity, std::initializer_list<int32_t> limits) {
  int i = 0;
  for (int32_t v : limits) {
    if (out && i < capacity) out[i] = v;
    ++i;
  }
  return i;
}

__device__ __forceinline__ int32_t clampi(int32_t c, int32_t hi) {
  return c < 0 ? 0 : (c > hi ? hi : c);
}

// Segment [lo, hi) of the row that entry i of row_ids names (empty for i >= count); ptr is
// clamped into [0, E] and the row into [0, num_rows): memory safety whatever the arrays hold.
__device__ __forceinline__ void clamped_segment(const int32_t* __restrict__ ptr,
                                                const int32_t* __restrict__ row_ids, int64_t i,
                                                int32_t count, int32_t num_rows, int64_t E,
                                                int64_t& lo, int64_t& hi) {
  lo = 0;
  hi = 0;
  if (i < count) {
    const int32_t r = clampi(row_ids[i], num_rows - 1);
    int64_t b = ptr[r], e = ptr[r + 1];
    b = b < 0 ? 0 : (b > E ? E : b);
    e = e < b ? b : (e > E ? E : e);
    lo = b;
    hi = e;
  }
}

// Segment [b, b + n) of row `row` of ptr, clamped into [0, E] so that a ptr that breaks the
// documented preconditions still indexes inside the arrays; n = 0 past num_rows.
__device__ __forceinline__ void row_segment(const int32_t* __restrict__ ptr, int64_t row,
                                            int32_t num_rows, int64_t E, int64_t& b, int32_t& n) {
  b = 0;
  n = 0;
  if (row < num_rows) {
    int64_t lo = ptr[row], hi = ptr[row + 1];
    lo = lo < 0 ? 0 : (lo > E ? E : lo);
    hi = hi < lo ? lo : (hi > E ? E : hi);
    b = lo;
    n = (int32_t)(hi - lo);
  }
}

// Forward work item: a run of whole destination rows [row0, row0+nrows) (or, nrows < 0, one
// segment of a long row whose partial sum is added atomically into a row pre-zeroed by
// zero_rows), with edge range [e0, e1) of the plan's permuted edge order (the task's CSR
// edges sorted by column).
struct FwdTask {
  int32_t row0;
  int32_t nrows;
  int32_t e0;
  int32_t e1;
};
static_assert(sizeof(FwdTask) == 16, "FwdTask is loaded as one dwordx4");

// Packed CBSR record size for k (k % 4 == 0): k f32 values + k u8 selectors, rounded to
// 64 B when that fits one 64-B sector, to one 128-B line when it fits one, else to 16 B
// (k = 32: 160-B records ran 2.73 ms against 3.24 ms for 256-B ones on Reddit).
inline int cbsr_record_bytes(int k) {
  const int b = 5 * k;
  return b <= 64 ? 64 : b <= 128 ? 128 : (b + 15) / 16 * 16;
}

// Forward records handed over by the caller (maxk_topk_cbsr_records writes them,
// maxk_spgemm_forward_records gathers them): layout as maxk_plan_info.fwd_layout 1, 2 or 4, one
// record every record_bytes from a 16-B aligned base. `need`: a null base is an error.
inline int check_records(const void* records, int64_t record_bytes, int layout, int k, bool need,
                         const char* who) {
  const std::string w(who);
  if (layout != 1 && layout != 2 && layout != 4) {
    set_error(w + ": layout must be 1, 2 or 4 (maxk_plan_info.fwd_layout)");
    return MAXK_ERR_UNSUPPORTED;
  }
  MAXK_CHECK_ARG(layout != 1 || k % 4 == 0, w + ": layout 1 needs k % 4 == 0");
  MAXK_CHECK_ARG(layout != 2 || (k + 2) / 3 <= kWave, w + ": layout 2 needs (k + 2) / 3 <= 64");
  MAXK_CHECK_ARG(layout != 4 || (k % 2 == 0 && k / 2 <= kWave),
                 w + ": layout 4 needs an even k with k / 2 <= 64");
  const int64_t bytes = layout == 1 ? 5 * (int64_t)k : 16 * (int64_t)((k + (layout == 2 ? 2 : 1)) /
                                                                      (layout == 2 ? 3 : 2));
  MAXK_CHECK_ARG(record_bytes % 16 == 0 && record_bytes >= bytes && record_bytes <= INT32_MAX,
                 w + ": record_bytes must be a multiple of 16 that holds the row's record");
  MAXK_CHECK_ARG((reinterpret_cast<uintptr_t>(records) & 15) == 0,
                 w + ": records must be 16-B aligned");
  MAXK_CHECK_ARG(records || !need, w + ": records is null");
  return MAXK_OK;
}

// Backward work item: edges [e0, e1) of the column-block-major, row-sorted edge list, all
// with source column in [col0, col0 + ncols). shared != 0: the block is split over several
// work-groups, so its LDS accumulator is flushed with float atomics into a pre-zeroed
// grad_sp; otherwise it is stored.
struct BwdTask {
  int32_t col0;
  int32_t ncols;
  int32_t e0;
  int32_t e1;
  int32_t shared;
  int32_t group;  // selector slot group (packed path): slots [group * k/S, (group+1) * k/S)
  int32_t chunk;  // piece index within its block (0 .. pieces - 1)
  int32_t slab;   // slab flush: float offset of this piece's [C][k] slab region; -1: piece
                  // 0 (stores straight into grad_sp)
};
static_assert(sizeof(BwdTask) == 32, "BwdTask is 2 x dwordx4");


__device__ __forceinline__ void lds_add(double* p, double v) {
  // ds_add_f64 (no return).
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void global_add(float* p, float v) {
  // One global_atomic_add_f32 (no CAS loop on gfx950).
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace maxk

// Opaque plan (definition shared by plan.hip and the kernels' launchers).
struct maxk_plan {
  int32_t num_nodes = 0;   // destination rows
  int32_t num_cols = 0;    // source columns (rows of the CBSR tables / grad_sp)
  int64_t num_edges = 0;
  int32_t dim_origin = 0;
  int32_t dim_k = 0;
  const int32_t* src_ptr = nullptr;  // identity of the graph the plan was built for
  const int32_t* src_idx = nullptr;
  int32_t cus = 256;             // compute units of the device the plan was built on
  // ---- forward: tiles of whole rows (FwdTask), edges column-sorted per tile
  int32_t fwd_tile_rows = 32;
  int32_t fwd_waves = 4;        // wavefronts per forward work-group (4 or 8)
  int32_t fwd_unroll = 8;       // forward sub-steps in flight per wave (4 only with 8 waves)
  int32_t fwd_rec_bytes = 0;     // packed CBSR record size (per-call pack)
  maxk::DeviceBuf<uint8_t> fwd_rec;  // [num_cols][fwd_rec_bytes] plan-owned workspace
  // fixed-point forward (LdsFix): per task {sexp, gexp} (fwd_fix_stats_kernel); the call's
  // {max |x|, min |x|} words live at fwd_xstat_off of the forward workspace
  int32_t fwd_fixed = 0;
  maxk::DeviceBuf<int2> fwd_fix;
  maxk::DeviceBuf<int32_t> fwd_rowptr;  // plan copy of ptr for the bounds' row sums
  int64_t fwd_xstat_off = 0;
  maxk::DeviceBuf<maxk::FwdTask> fwd_tasks;  // e0/e1 index the permuted edge order below
  int32_t fwd_phases = 1;        // column windows of the rotated sweep (1: no rotation)
  int32_t fwd_rot_ticks = 0;     // > 0: rotated sweeps, s_memrealtime ticks per window
  int32_t fwd_chunk3 = 0;        // lane-chunk records: 3 values + their selectors per 16 B
  int32_t fwd_chunk2 = 0;        // pair-chunk records: 2 values + their selectors per 16 B
  int32_t fwd_quad = 0;          // quad-shared edge-word loads
  int32_t fwd_two_tables = 0;    // gather from sp_data / sp_index directly (no pack)
  maxk::DeviceBuf<int32_t> fwd_phase_off;  // [tasks][phases + 1] edge offsets per window
  maxk::DeviceBuf<int32_t> fwd_perm;  // CSR edge id of each permuted forward edge
  maxk::DeviceBuf<uint2> fwd_cv;  // {column | (row within the task << kFwdColBits), val bits}
  // Row-constant edge values (every edge of a destination row carries the same finite nonzero
  // value, bit for bit: SAGE mean, sum / GIN, any row-normalised adjacency): fwd_cv4 holds the
  // column | row words alone, [E + 1] in the same order, fwd_rowval [N] the row's value (1 for
  // an edgeless row), fwd_cv is released and fwd_fix is computed for unit weights. The
  // fixed-point forward then sums x with weight 1 and scales each row sum once (its f64 fallback
  // weighs each term with fwd_rowval of the word's row). Detected at plan build and at every
  // maxk_plan_refresh_values, which switches the stream either way (plan.hip).
  int32_t fwd_rowconst = 0;
  int32_t fwd_rowconst_off = 0;  // maxk_plan_options.fwd_rowconst == 2: always the 8-byte words
  maxk::DeviceBuf<uint32_t> fwd_cv4;
  maxk::DeviceBuf<float> fwd_rowval;
  int32_t n_fwd_tasks = 0;
  maxk::DeviceBuf<int32_t> zero_rows;  // rows written by split tasks (atomic), zeroed first
  int32_t n_zero_rows = 0;
  // ---- backward, column blocks (sspmm_bwd4_kernel): one 12-B record per reordered edge
  // {row * D * 4 (or the row index when grad_out exceeds 4 GiB), column within its block,
  // val}; F selector slots per lane, S slot groups, k padded to bwd_kp (a multiple of F * S;
  // the padding slots gather feature 0 into accumulators that are never stored)
  int32_t bwd_feats = 4;         // F: 4 or 2
  int32_t bwd_slot_groups = 1;   // S
  int32_t bwd_kp = 0;            // padded slots per column
  int32_t bwd_ks = 0;            // accumulator floats per column and group (= bwd_kp / S)
  int32_t bwd_unroll = 8;
  int32_t bwd_waves = 8;
  int32_t bwd_big = 0;           // grad_out > 4 GiB: 64-bit row addressing
  int32_t bwd_block_cols = 0;
  int32_t n_bwd_blocks = 0;
  maxk::DeviceBuf<maxk::BwdTask> bwd_tasks;
  int32_t n_bwd_tasks = 0;
  int32_t n_bwd_shared = 0;
  maxk::DeviceBuf<int32_t> bwd_perm;  // CSR edge id of each reordered edge
  maxk::DeviceBuf<uint32_t> bwd_rec;  // [num_edges + kBwdRecPad][3]
  maxk::DeviceBuf<uint32_t> bwd_sel;  // plan-owned workspace: the slabs (bwd_slab_floats)
  // two-pass backward (low row reuse): a row pass writes each edge's k products val *
  // grad_out[r, sel(c)] into the edge's slot of bwd_tbuf (CSR order), a column pass sums the
  // slots of each column's in-edges (bwd_perm, bwd_colptr)
  int32_t bwd_twopass = 0;
  int32_t bwd_tp_rows = 1;       // R: destination rows per wavefront of the row pass
  maxk::DeviceBuf<uint32_t> bwd_erec;  // [num_edges][2] CSR order: {column | (row % R) << 26, val}
  maxk::DeviceBuf<float> bwd_tbuf;  // [max chunk edges][k] plan-owned workspace
  maxk::DeviceBuf<int32_t> bwd_colptr;  // [num_cols + 1] offsets of the column-sorted edges
  // row chunks of the two-pass backward (workspace bounded by kBwdTwoPassWorkspaceCap):
  // chunk p covers destination rows [tp_rows[p], tp_rows[p+1]) = CSR edges [tp_edges[p],
  // tp_edges[p+1]); bwd_colptr2[p * NC + c] = first column-sorted position of column c whose
  // row is >= tp_rows[p] (rows ascend within a column), p = 0 .. P (P = 1: bwd_colptr)
  int32_t bwd_tp_chunks = 1;
  std::vector<int32_t> tp_rows;
  std::vector<int64_t> tp_edges;
  maxk::DeviceBuf<int32_t> bwd_colptr2;
  // column order of the column blocks (maxk_plan_options.col_order): bwd_corder[p] = the
  // source column placed at position p of the blocks (nullptr: identity)
  int32_t col_order = 1;
  maxk::DeviceBuf<int32_t> bwd_corder;
  // slab flush of split blocks: piece 0 of a block stores into grad_sp, piece p > 0 into its
  // [C][k] slab region (bwd_slab_floats f32 in all, at byte bwd_slab_off of the backward
  // workspace, behind the selector words); bwd_combine_kernel adds each block's regions in
  // piece order. bwd_combine: one int4 {slab offset, regions, col0, ncols} per block with
  // more than one piece. bwd_slab_floats == 0 with split blocks: global float atomics
  int64_t bwd_slab_floats = 0;
  int64_t bwd_slab_off = 0;
  maxk::DeviceBuf<int4> bwd_combine;
  int32_t n_bwd_combine = 0;
  int64_t device_bytes = 0;
  // per-call scratch: the forward's packed CBSR records and statistics words, the backward's
  // selector words + flush slabs or two-pass product workspace. external_ws: the plan
  // allocates none of them and the *_ws entry points take the caller's buffer
  int32_t external_ws = 0;
  int64_t fwd_ws_bytes = 0;
  int64_t bwd_ws_bytes = 0;
  int32_t bwd_row_order = 1;     // rows in the block streams: 1 ascending, 2 scattered
  // windows of the forward / column-block backward waves: 1 static interleave, 2 handed out
  // by a per-work-group LDS counter (maxk_plan_options.fwd_handout / bwd_handout)
  int32_t fwd_handout = 1;
  int32_t bwd_handout = 1;
};

// maxk_plan_info.fwd_layout: what the plan's forward gathers from (maxk_hip.h).
inline int plan_fwd_layout(const maxk_plan* p) {
  if (p->fwd_chunk2) return 4;
  if (p->fwd_chunk3) return 2;
  if (p->dim_k % 4 != 0) return 3;
  return p->fwd_two_tables ? 0 : 1;
}

// The plan's forward kernel, with 8-byte or 4-byte edge words.
inline maxk::FwdVariant plan_fwd_variant(const maxk_plan* p, bool rowconst) {
  return maxk::select_fwd_variant(plan_fwd_layout(p), p->dim_k, p->fwd_fix != nullptr,
                                  p->fwd_quad != 0, p->fwd_waves, p->fwd_unroll, rowconst);
}

// Whether the plan's forward kernel has a 4-byte edge-word form.
inline bool plan_fwd_rowconst_shape(const maxk_plan* p) {
  return !(plan_fwd_variant(p, true) == maxk::kFwdNoRowconst);
}
