// Host-only soundness run of the plan build's host stages (tooling, not product): the forward
// task list, the kernel shape selection and the column-block chunk count, over random row
// pointers and block offsets, without a device. Meant for a CPU build with the host sanitizers:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//     -Iinclude -Ispgemm-gnn_amd/csrc tools/plan_host_check.hip -o tools/plan_host_check
//
// It includes plan.hip to reach its file-local stages and checks what must hold of their output:
// the forward tasks cover every row and every edge exactly once, split rows are listed in
// zero_rows, the shapes are ones that have a kernel, the chunk count is at least 1.
#include <cstdio>
#include <cstdlib>

#include "../spgemm-gnn_amd/csrc/plan.hip"

namespace maxk {
void set_error(const std::string& msg) { std::fprintf(stderr, "error: %s\n", msg.c_str()); }
}  // namespace maxk

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

static uint64_t g_seed = 1;
static uint32_t rnd() {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_seed >> 33);
}

static void check_fwd_tasks(const std::vector<int32_t>& hp, int N, int R, int64_t cap) {
  std::vector<FwdTask> tasks;
  std::vector<int32_t> zrows;
  build_fwd_tasks(hp, N, R, cap, tasks, zrows);
  std::vector<int> rows(N, 0);
  std::vector<int> edges(hp[N], 0);
  size_t split_rows = 0;
  for (const FwdTask& t : tasks) {
    CHECK(t.row0 >= 0 && t.row0 < N && t.e0 >= 0 && t.e0 <= t.e1 && t.e1 <= hp[N]);
    if (t.nrows < 0) {  // a segment of a split row
      CHECK(t.e0 >= hp[t.row0] && t.e1 <= hp[t.row0 + 1]);
      if (t.e0 == hp[t.row0]) { ++rows[t.row0]; ++split_rows; }
    } else {
      CHECK(t.nrows >= 1 && t.nrows <= R && t.row0 + t.nrows <= N);
      CHECK(t.e0 == hp[t.row0] && t.e1 == hp[t.row0 + t.nrows]);
      for (int r = t.row0; r < t.row0 + t.nrows; ++r) ++rows[r];
    }
    for (int e = t.e0; e < t.e1; ++e) ++edges[e];
  }
  for (int r = 0; r < N; ++r) CHECK(rows[r] == 1);
  for (int c : edges) CHECK(c == 1);
  CHECK(zrows.size() == split_rows);
  for (int32_t r : zrows) CHECK(r >= 0 && r < N);
}

static void check_shapes_and_chunks(int N, int NC, int64_t E, int D, int k, int nblocks,
                                    const std::vector<int64_t>& offs) {
  maxk_plan_options o{};
  PlanBuild ctx{nullptr, nullptr, nullptr, N, NC, E, D, k, o, nullptr, nullptr};
  ctx.plan.reset(new maxk_plan());
  ctx.plan->cus = 256;
  choose_fwd_shape(ctx);
  choose_bwd_shape(ctx);
  const maxk_plan* p = ctx.plan.get();
  CHECK(p->fwd_tile_rows >= 1 && p->fwd_tile_rows <= kFwdMaxTileRows);
  // the shapes have a kernel: the variants they select are in the compiled tables
  CHECK(p->fwd_waves == 4 || p->fwd_waves == 8);
  CHECK(has_variant(kFwdVariants, plan_fwd_variant(p, false)));
  CHECK(!plan_fwd_rowconst_shape(p) || has_variant(kFwdVariants, plan_fwd_variant(p, true)));
  CHECK(p->bwd_feats == 2 || p->bwd_feats == 4);
  for (int big = 0; big < 2; ++big)
    CHECK(has_variant(kBwdVariants,
                      select_bwd_variant(p->bwd_feats, p->bwd_kp / p->bwd_slot_groups / p->bwd_feats,
                                         p->bwd_waves, p->bwd_unroll, big != 0)));
  CHECK(p->bwd_kp >= k && p->bwd_kp % (p->bwd_feats * p->bwd_slot_groups) == 0);
  CHECK(ctx.C >= 1 && ctx.C <= std::max(NC, 1) && ctx.S >= 1);
  if (nblocks > 0 && E > 0) {
    ctx.nblocks = nblocks;
    ctx.offs = offs;
    CHECK(bwd_chunk_count(ctx) >= 1);
  }
}

int main() {
  // forward task lists: random degrees with heavy rows, N = 0, E = 0, one row holding every edge
  for (int it = 0; it < 200; ++it) {
    const int N = it == 0 ? 0 : 1 + (int)(rnd() % 3000);
    const int mode = it % 4;  // 0 random, 1 no edges, 2 every edge in one row, 3 a few heavy rows
    std::vector<int32_t> hp(N + 1, 0);
    const int heavy = N ? (int)(rnd() % N) : 0;
    for (int r = 0; r < N; ++r) {
      int deg = 0;
      if (mode == 0) deg = (int)(rnd() % 64);
      if (mode == 2) deg = r == heavy ? 50000 : 0;
      if (mode == 3) deg = rnd() % 97 == 0 ? (int)(rnd() % 20000) : (int)(rnd() % 8);
      hp[r + 1] = hp[r] + deg;
    }
    const int R = 1 + (int)(rnd() % kFwdMaxTileRows);
    const int64_t cap = it % 3 == 0 ? 0 : 1 + (int64_t)(rnd() % 5000);
    check_fwd_tasks(hp, N, R, cap);
  }
  // shapes and chunk counts: random sizes and block offsets, a zero-edge block, one block
  // holding every edge, N = 0, E = 0
  const int ks[] = {1, 2, 7, 8, 12, 16, 24, 32, 48, 64, 100, 128, 192, 250, 256};
  for (int it = 0; it < 400; ++it) {
    const int D = 256;
    const int k = ks[rnd() % (sizeof(ks) / sizeof(ks[0]))];
    const int N = it % 17 == 0 ? 0 : 1 + (int)(rnd() % 200000);
    const int NC = N == 0 ? 0 : 1 + (int)(rnd() % 200000);
    const int64_t E = (N == 0 || it % 13 == 0) ? 0 : 1 + (int64_t)(rnd() % 20000000);
    const int nblocks = NC ? 1 + (int)(rnd() % 512) : 0;
    std::vector<int64_t> offs(nblocks + 1, 0);
    if (nblocks > 0) {
      const int mode = it % 3;  // 0 random cuts, 1 every edge in one block, 2 an empty first block
      for (int b = 1; b < nblocks; ++b)
        offs[b] = mode == 1 ? (b > nblocks / 2 ? E : 0) : (int64_t)(rnd() % (uint64_t)(E + 1));
      if (mode == 2 && nblocks > 1) offs[1] = 0;
      offs[nblocks] = E;
      std::sort(offs.begin(), offs.end());
    }
    check_shapes_and_chunks(N, NC, E, D, k, nblocks, offs);
  }
  std::puts("plan host check ok");
  return 0;
}
