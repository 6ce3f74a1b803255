// Plan digest (tooling, not product): builds a plan for each of a fixed list of small host-made
// graphs through maxk_plan_create_sized and prints, per case, every scalar of maxk_plan (but the
// two caller pointers), tp_rows / tp_edges, the non-nullness of the 18 plan arrays and, for
// every array that the build initialises (all but the workspaces fwd_rec, bwd_sel, bwd_tbuf), its
// element count and the FNV-1a hash of its whole allocated extent. Two builds of plan.hip that
// produce the same plans print the same text (profiles/plan_digest_mi355x.txt).
//
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -Iinclude -Ispgemm-gnn_amd/csrc \
//     tools/plan_digest.hip -o tools/plan_digest -Lspgemm-gnn_amd/maxk_kernels -lmaxk_hip \
//     -Wl,-rpath,'$ORIGIN/../spgemm-gnn_amd/maxk_kernels'
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "common.h"

using maxk::kBwdRecPad;

namespace {

struct Graph {
  int32_t N = 0, NC = 0;
  std::vector<int32_t> ptr{0}, idx;
  std::vector<float> val;
};

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};

// Rows with deg(r) edges each into columns drawn from [lo(r), hi(r)), sorted within the row.
template <class Deg, class Lo, class Hi>
Graph make_graph(int32_t N, int32_t NC, uint64_t seed, Deg deg, Lo lo, Hi hi) {
  Graph g;
  g.N = N;
  g.NC = NC;
  Rng rng{seed};
  for (int32_t r = 0; r < N; ++r) {
    const int d = deg(r);
    const size_t e0 = g.idx.size();
    for (int i = 0; i < d; ++i) g.idx.push_back(lo(r) + (int32_t)(rng.next() % (uint32_t)(hi(r) - lo(r))));
    std::sort(g.idx.begin() + e0, g.idx.end());
    for (int i = 0; i < d; ++i) g.val.push_back((float)(1 + rng.next() % 1000) / 1024.0f);
    g.ptr.push_back((int32_t)g.idx.size());
  }
  return g;
}

Graph uniform(int32_t N, int32_t NC, int per_row, uint64_t seed) {
  return make_graph(N, NC, seed, [=](int) { return per_row; }, [](int) { return 0; },
                    [=](int) { return NC; });
}

uint64_t fnv1a(const uint8_t* b, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

#define HIP_OK(expr)                                                             \
  do {                                                                           \
    const hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) {                                                      \
      std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(_e));            \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

template <class T>
T* upload(const std::vector<T>& v) {
  T* d = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&d), std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}

// One array line: non-nullness, and with elem > 0 its element count and the hash of its extent.
void array_line(const char* name, const void* d, int64_t count, size_t elem) {
  if (!d) {
    std::printf("  %-14s null\n", name);
  } else if (elem == 0) {
    std::printf("  %-14s set (workspace)\n", name);
  } else {
    std::vector<uint8_t> h((size_t)count * elem);
    if (!h.empty()) HIP_OK(hipMemcpy(h.data(), d, h.size(), hipMemcpyDeviceToHost));
    std::printf("  %-14s set n=%lld fnv=%016llx\n", name, (long long)count,
                (unsigned long long)fnv1a(h.data(), h.size()));
  }
}

void digest(const char* name, const Graph& g, int32_t D, int32_t k, const maxk_plan_options& o,
            const std::vector<int32_t>* order = nullptr) {
  const int64_t E = (int64_t)g.idx.size();
  int32_t* d_ptr = upload(g.ptr);
  int32_t* d_idx = upload(g.idx);
  float* d_val = upload(g.val);
  int32_t* d_order = order ? upload(*order) : nullptr;
  maxk_plan* p = nullptr;
  const int rc = maxk_plan_create_sized(d_ptr, d_idx, d_val, g.N, g.NC, E, D, k, &o,
                                        (int64_t)sizeof(o), d_order, nullptr, &p);
  std::printf("case %s: N=%d NC=%d E=%lld D=%d k=%d rc=%d\n", name, g.N, g.NC, (long long)E, D, k, rc);
  if (rc != MAXK_OK) {
    std::printf("  error: %s\n", maxk_last_error());
    std::exit(1);
  }
  HIP_OK(hipDeviceSynchronize());
#define S(f) std::printf("  %-16s %lld\n", #f, (long long)p->f)
  S(num_nodes); S(num_cols); S(num_edges); S(dim_origin); S(dim_k); S(cus);
  S(fwd_tile_rows); S(fwd_waves); S(fwd_unroll); S(fwd_rec_bytes); S(fwd_fixed); S(fwd_xstat_off);
  S(fwd_phases); S(fwd_rot_ticks); S(fwd_chunk3); S(fwd_chunk2); S(fwd_quad); S(fwd_two_tables);
  S(n_fwd_tasks); S(n_zero_rows); S(fwd_rowconst);
  S(bwd_feats); S(bwd_slot_groups); S(bwd_kp); S(bwd_ks); S(bwd_unroll); S(bwd_waves); S(bwd_big);
  S(bwd_block_cols); S(n_bwd_blocks); S(n_bwd_tasks); S(n_bwd_shared);
  S(bwd_twopass); S(bwd_tp_rows); S(bwd_tp_chunks); S(col_order);
  S(bwd_slab_floats); S(bwd_slab_off); S(n_bwd_combine); S(device_bytes);
  S(external_ws); S(fwd_ws_bytes); S(bwd_ws_bytes); S(bwd_row_order); S(fwd_handout); S(bwd_handout);
#undef S
  std::printf("  tp_rows         ");
  for (int32_t r : p->tp_rows) std::printf(" %d", r);
  std::printf("\n  tp_edges        ");
  for (int64_t e : p->tp_edges) std::printf(" %lld", (long long)e);
  std::printf("\n");
  const int64_t nt = p->n_fwd_tasks, P = p->bwd_tp_chunks;
  array_line("fwd_tasks", p->fwd_tasks, nt, sizeof(maxk::FwdTask));
  array_line("fwd_rec", p->fwd_rec, 0, 0);
  array_line("fwd_perm", p->fwd_perm, E, 4);
  array_line("fwd_cv", p->fwd_cv, E + 1, 8);
  array_line("fwd_cv4", p->fwd_cv4, E + 1, 4);
  array_line("fwd_rowval", p->fwd_rowval, (int64_t)g.N, 4);
  array_line("fwd_fix", p->fwd_fix, nt, 8);
  array_line("fwd_rowptr", p->fwd_rowptr, (int64_t)g.N + 1, 4);
  array_line("fwd_phase_off", p->fwd_phase_off, nt * (p->fwd_phases + 1), 4);
  array_line("zero_rows", p->zero_rows, p->n_zero_rows, 4);
  array_line("bwd_tasks", p->bwd_tasks, p->n_bwd_tasks, sizeof(maxk::BwdTask));
  array_line("bwd_perm", p->bwd_perm, E, 4);
  array_line("bwd_rec", p->bwd_rec, 3 * (E + kBwdRecPad), 4);
  array_line("bwd_sel", p->bwd_sel, 0, 0);
  array_line("bwd_colptr", p->bwd_colptr, (int64_t)p->n_bwd_blocks + 1, 4);
  array_line("bwd_erec", p->bwd_erec, 2 * E, 4);
  array_line("bwd_tbuf", p->bwd_tbuf, 0, 0);
  array_line("bwd_combine", p->bwd_combine, p->n_bwd_combine, 16);
  array_line("bwd_colptr2", p->bwd_colptr2, (P + 1) * g.NC, 4);
  array_line("bwd_corder", p->bwd_corder, g.NC, 4);
  maxk_plan_destroy(p);
  HIP_OK(hipFree(d_ptr));
  HIP_OK(hipFree(d_idx));
  HIP_OK(hipFree(d_val));
  if (d_order) HIP_OK(hipFree(d_order));
}

maxk_plan_options opts() { return maxk_plan_options{}; }

}  // namespace

int main() {
  const Graph u = uniform(3000, 3000, 30, 11);
  const int32_t E = (int32_t)u.idx.size();
  maxk_plan_options o;

  for (int k : {8, 12, 16, 32, 64}) digest(("uniform_k" + std::to_string(k)).c_str(), u, 64, k, opts());
  o = opts(); o.fwd_fixed = 2;
  digest("uniform_k16_float", u, 64, 16, o);
  o = opts(); o.fwd_fixed = 1;
  digest("uniform_k8_fixed", u, 64, 8, o);
  o = opts(); o.fwd_two_tables = 2;
  digest("uniform_k32_packed", u, 64, 32, o);
  digest("uniform_k250_d256", u, 256, 250, opts());

  // one row holds a third of the edges; the cap splits it over 15 tasks
  const Graph heavy = make_graph(3000, 3000, 12, [](int r) { return r == 1500 ? 30000 : 20; },
                                 [](int) { return 0; }, [](int) { return 3000; });
  o = opts(); o.fwd_task_cap = 2048;
  digest("heavy_row", heavy, 64, 16, o);

  for (int ext : {0, 1}) {
    o = opts(); o.bwd_algo = 1; o.bwd_piece_edges = E / 400; o.external_workspace = ext;
    digest(ext ? "slabs_external_ws" : "slabs_owned_ws", u, 64, 16, o);
  }
  for (int chunks : {1, 7})
    for (int ext : {0, 1}) {
      o = opts(); o.bwd_algo = 3; o.bwd_tp_chunks = chunks; o.external_workspace = ext;
      digest(("two_pass_" + std::to_string(chunks) + (ext ? "_external_ws" : "_owned_ws")).c_str(),
             u, 64, 16, o);
    }

  o = opts(); o.bwd_algo = 1; o.col_order = 2;
  digest("col_order_scattered", u, 64, 16, o);
  std::vector<int32_t> given(u.NC);
  for (int32_t c = 0; c < u.NC; ++c) given[c] = (int32_t)(((int64_t)c * 1013 + 17) % u.NC);  // gcd(1013, 3000) = 1
  o = opts(); o.bwd_algo = 1; o.col_order = 4;
  digest("col_order_given", u, 64, 16, o, &given);
  // the same on many small column blocks
  o = opts(); o.bwd_algo = 1; o.col_order = 2; o.bwd_lds_bytes = 4096;
  digest("col_order_scattered_small_blocks", u, 64, 16, o);

  o = opts(); o.bwd_row_order = 2;
  digest("row_order_scattered", u, 64, 16, o);
  o = opts(); o.bwd_row_order = 1;
  digest("row_order_ascending", u, 64, 16, o);
  for (int ro : {0, 1, 2}) {
    o = opts(); o.bwd_algo = 1; o.bwd_row_order = ro; o.bwd_lds_bytes = 4096;
    digest(("small_blocks_row_order_" + std::to_string(ro)).c_str(), u, 64, 16, o);
  }

  digest("rect", uniform(3000, 2000, 30, 13), 64, 16, opts());
  digest("no_edges", uniform(3000, 3000, 0, 14), 64, 8, opts());
  digest("no_nodes", Graph{}, 64, 8, opts());

  // two ID-ordered communities, 40 edges per row: the automatic row order scatters the rows
  const int32_t CN = 4000;
  const Graph comm = make_graph(CN, CN, 15, [](int) { return 40; },
                                [=](int r) { return r < CN / 2 ? 0 : CN / 2; },
                                [=](int r) { return r < CN / 2 ? CN / 2 : CN; });
  digest("communities_auto_row_order", comm, 64, 16, opts());
  o = opts(); o.bwd_lds_bytes = 16384;
  digest("communities_auto_row_order_small_blocks", comm, 64, 16, o);
  return 0;
}
