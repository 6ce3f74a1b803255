// Body of gat_attention_fwd_kernel and of its head-batched twin (gat_attention.hip), included in both so
// that the single-head kernel is compiled from exactly the statements it always had.
  __shared__ float red[2 * kEsWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kEsTileRows;
  const int32_t col_hi = num_cols - 1;

  int64_t b;
  int32_t n;
  const int64_t row = row0 + wave * kEsWaveRows + lane / kEsGroup;
  row_segment(ptr, row, num_rows, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  if (__ballot(ns > 0) != 0) {
    // a group with no short row scores edge 0 (E > 0) and writes nothing
    const int64_t bs = ns > 0 ? b : 0;
    const GatScore src{idx + bs, el, gat_row_score(er, row, num_rows), slope, col_hi};
    es_fwd_regs<kEsGroup, kEsShortSlots>(src, out + bs, ns, lane % kEsGroup);
  }
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    const GatScore src{idx + bg, el, er[row0 + wave * kEsWaveRows + g], slope, col_hi};
    es_fwd_medium(src, out + bg, ng, lane);
  }

  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    row_segment(ptr, row0 + r, num_rows, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    const GatScore src{idx + bh, el, er[row0 + r], slope, col_hi};
    es_fwd_hub<true>(src, out + bh, nh, tid, lane, wave, red);
  }
