// Softmax of per-edge logits over each destination row's in-edges, and its gradient
// (include/maxk_hip.h, "Edge softmax").
//
//   forward   m = max x_e,  p_e = expf(x_e - m),  s = sum p_e,  out_e = p_e * (1 / s)
//   backward  t = sum y_e * g_e,  grad_e = y_e * (g_e - t)
//
// A CSR row is one contiguous segment of ptr, so both are pure streaming kernels with a
// reduction per segment: no atomics, no scratch, no plan.
//
// Shape: one 256-thread work-group per tile of kEsTileRows consecutive rows; wave w of the
// group owns rows 4w .. 4w + 3 of the tile. A row is served by its length n alone:
//   * short,  n <= kEsShortMax (64): by 16 lanes (the four rows of a wave side by side), four
//     elements per lane in registers, 4-level xor butterflies;
//   * medium, n <= kEsMediumMax (1024): by its wave, S = 2, 4, 8 or 16 elements per lane in
//     registers (the smallest S with 64 S >= n), read once and written once;
//   * hub, above: by the whole work-group that owns its tile, every thread striding the segment
//     by 256, waves combined through LDS; the segment is read again per pass (two extra reads
//     forward, one backward) out of the L2, which a segment of this size has just filled.
// Hub rows reach a work-group with no list of them: every thread of the group reads the tile's
// row lengths, so the group agrees on its hubs and takes them together after its waves' own
// rows. A 20,000-edge hub is 80 KB, microseconds for one work-group, and the 16-row tiles of a
// graph outnumber the CUs by far, so the dispatcher levels the difference.
// Element j of a row always sits in lane j % W, slot j / W (W = 16, 64 or 256 by the row's
// length): a lane sums its slots in order, then the butterfly. Position, neighbours, the
// segment's alignment and num_rows never enter, so a row's bits depend on its values and length.
// Loads are one dword per lane, 64 contiguous lanes: vector loads would tie the order to
// ptr[r] % 4.
// The device functions are shared with gat_attention.hip (edge_softmax.h): here their source is
// the logits array.
#include "edge_softmax.h"

// every product, difference and sum below is one IEEE operation
#pragma clang fp contract(off)

namespace maxk {

// ---------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(kEsThreads) void edge_softmax_fwd_kernel(
    const int32_t* __restrict__ ptr, const float* __restrict__ logits, float* __restrict__ out,
    int32_t num_rows, int64_t E) {
  __shared__ float red[2 * kEsWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kEsTileRows;

  // the wave's own rows: short ones side by side, medium ones one after the other
  int64_t b;
  int32_t n;
  row_segment(ptr, row0 + wave * kEsWaveRows + lane / kEsGroup, num_rows, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  if (__ballot(ns > 0) != 0) {
    // a group with no short row reads element 0 (E > 0) and writes nothing
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

  // the tile's hub rows: every thread reads the same lengths, so the branch is group-uniform
  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    row_segment(ptr, row0 + r, num_rows, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    es_fwd_hub(EsArray{logits + bh}, out + bh, nh, tid, lane, wave, red);
  }
}

// --------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(kEsThreads) void edge_softmax_bwd_kernel(
    const int32_t* __restrict__ ptr, const float* __restrict__ y, const float* __restrict__ gy,
    float* __restrict__ out, int32_t num_rows, int64_t E) {
  __shared__ float red[kEsWaves];
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
// Checks shared by both directions: `ins` are the nin f32 [E] inputs.
static int es_check(const std::string& w, const int32_t* ptr, const float* const* ins, int nin,
                    const float* out, int32_t N, int64_t E) {
  MAXK_CHECK_ARG(N >= 0 && E >= 0 && E <= (int64_t)INT32_MAX, w + "sizes out of range");
  if (E == 0 || N == 0) return MAXK_OK;
  bool null = !ptr || !out;
  for (int i = 0; i < nin; ++i) null = null || !ins[i];
  MAXK_CHECK_ARG(!null, w + "null pointer");
  bool overlap = ranges_overlap(out, 4 * E, ptr, 4 * ((int64_t)N + 1));
  for (int i = 0; i < nin; ++i) overlap = overlap || ranges_overlap(out, 4 * E, ins[i], 4 * E);
  MAXK_CHECK_ARG(!overlap, w + "the output overlaps an input");
  return MAXK_OK;
}

}  // namespace maxk

extern "C" int maxk_edge_softmax_forward(const int32_t* ptr, const float* logits, float* out,
                                         int32_t num_rows, int64_t num_edges, void* stream) {
  using namespace maxk;
  const float* ins[1] = {logits};
  const int rc = es_check("maxk_edge_softmax_forward: ", ptr, ins, 1, out, num_rows, num_edges);
  if (rc != MAXK_OK || num_edges == 0 || num_rows == 0) return rc;
  hipLaunchKernelGGL(edge_softmax_fwd_kernel, es_grid(num_rows), dim3(kEsThreads), 0,
                     (hipStream_t)stream, ptr, logits, out, num_rows, num_edges);
  MAXK_LAUNCH_CHECK("maxk_edge_softmax_forward launch");
  return MAXK_OK;
}

extern "C" int maxk_edge_softmax_backward(const int32_t* ptr, const float* y, const float* grad_y,
                                          float* grad_logits, int32_t num_rows, int64_t num_edges,
                                          void* stream) {
  using namespace maxk;
  const float* ins[2] = {y, grad_y};
  const int rc =
      es_check("maxk_edge_softmax_backward: ", ptr, ins, 2, grad_logits, num_rows, num_edges);
  if (rc != MAXK_OK || num_edges == 0 || num_rows == 0) return rc;
  hipLaunchKernelGGL(edge_softmax_bwd_kernel, es_grid(num_rows), dim3(kEsThreads), 0,
                     (hipStream_t)stream, ptr, y, grad_y, grad_logits, num_rows, num_edges);
  MAXK_LAUNCH_CHECK("maxk_edge_softmax_backward launch");
  return MAXK_OK;
}

extern "C" int maxk_edge_softmax_row_limits(int32_t* out, int32_t capacity) {
  return maxk::copy_limits(out, capacity, {maxk::kEsShortMax, maxk::kEsMediumMax});
}
