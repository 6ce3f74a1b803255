// Body of edge_colsum_kernel and of its head-batched twin (gat_attention.hip), included in both so
// that the single-head kernel is compiled from exactly the statements it always had.
  __shared__ float red[kEsWaves];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t col0 = (int64_t)blockIdx.x * kEsTileRows;
  const int32_t edge_hi = (int32_t)(E - 1);

  int64_t b;
  int32_t n;
  const int64_t col = col0 + wave * kEsWaveRows + lane / kEsGroup;
  row_segment(ptr_t, col, num_cols, E, b, n);
  const int32_t ns = n <= kEsShortMax ? n : 0;
  float s = 0.f;
  if (__ballot(ns > 0) != 0) {
    const int64_t bs = ns > 0 ? b : 0;
    s = es_sum_regs<kEsGroup, kEsShortSlots>(GatPermuted{order + bs, values, edge_hi}, ns,
                                             lane % kEsGroup);
  }
  if (col < num_cols && n <= kEsShortMax && lane % kEsGroup == 0) out[col] = s;
#pragma unroll
  for (int g = 0; g < kEsWaveRows; ++g) {
    const int32_t ng = __shfl(n, g * kEsGroup, kWave);
    if (ng <= kEsShortMax || ng > kEsMediumMax) continue;  // wave-uniform
    const int64_t bg = __shfl(b, g * kEsGroup, kWave);
    const float sg = es_sum_medium(GatPermuted{order + bg, values, edge_hi}, ng, lane);
    if (lane == 0) out[col0 + wave * kEsWaveRows + g] = sg;
  }

  for (int r = 0; r < kEsTileRows; ++r) {
    int64_t bh;
    int32_t nh;
    row_segment(ptr_t, col0 + r, num_cols, E, bh, nh);
    if (nh <= kEsMediumMax) continue;
    const GatPermuted src{order + bh, values, edge_hi};
    float a = 0.f;
#pragma unroll kEsHubUnroll
    for (int32_t j = tid; j < nh; j += kEsThreads) a = a + src(j);
    const float sh = es_hub_combine(a, lane, wave, red);
    if (tid == 0) out[col0 + r] = sh;
    __syncthreads();  // red is free for the tile's next hub
  }
