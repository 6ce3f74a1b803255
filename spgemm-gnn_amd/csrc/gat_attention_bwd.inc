// Body of gat_attention_bwd_kernel and of its head-batched twin (gat_attention.hip), included in both so
// that the single-head kernel is compiled from exactly the statements it always had.
  __shared__ float red[kEsWaves];
  __shared__ float red2[kEsWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t row0 = (int64_t)blockIdx.x * kEsTileRows;
  const int32_t col_hi = num_cols - 1;

  int64_t b;
  int32_t n;
  const int64_t row = row0 + wave * kEsWaveRows + lane / kEsGroup;
  row_segment(ptr, row, num_rows, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  float s = 0.f;
  if (__ballot(ns > 0) != 0) {
    const int64_t bs = ns > 0 ? b : 0;
    const GatScore post{idx + bs, el, gat_row_score(er, row, num_rows), slope, col_hi};
    s = es_sum<kEsGroup>(es_bwd_regs<kEsGroup, kEsShortSlots>(y + bs, gy + bs, out + bs, ns,
                                                              lane % kEsGroup, post));
  }
  if (row < num_rows && n <= kEsShortMax && lane % kEsGroup == 0) grad_er[row] = s;
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    const int64_t rg = row0 + wave * kEsWaveRows + g;
    const GatScore post{idx + bg, el, er[rg], slope, col_hi};
    const float sg = es_sum<kWave>(es_bwd_medium(y + bg, gy + bg, out + bg, ng, lane, post));
    if (lane == 0) grad_er[rg] = sg;
  }

  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    row_segment(ptr, row0 + r, num_rows, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    const GatScore post{idx + bh, el, er[row0 + r], slope, col_hi};
    const float acc = es_bwd_hub(y + bh, gy + bh, out + bh, nh, tid, lane, wave, red, post);
    const float sh = es_hub_combine(acc, lane, wave, red2);  // its barrier frees red
    if (tid == 0) grad_er[row0 + r] = sh;
    // red2 is written again only behind the next hub's first barrier
  }
