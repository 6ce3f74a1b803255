"""Where a MaxK aggregation autograd step spends its time (tooling, round 5): Reddit-shaped bench
graph, D = 256, k = 16 (or --k), x [N, D] requiring grad; one step = maxk_aggregate(x, graph, k)
forward + backward with a given upstream gradient. Prints the step's device time (HIP events),
the host time per step (wall clock of the Python calls without synchronising, i.e. how long
the CPU takes to queue it), and the kernel times of its parts measured alone: top-k, SpGEMM,
SSpMM, MaxK scatter. Round 6: also the unfused composition (MaxKFunction -> SpGEMMFunction,
whose forward packs / scans the tables) in the same process, and the fused parts (top-k with
statistics in the plan's layout, forward given the statistics). Round 7: where the plan's forward
gathers records (fwd_layout 1, 2, 4) the fused parts are the ones maxk_aggregate runs: the top-k
writing the records and a plain selector table (statistics only for a fixed-point forward),
and the forward gathering those records (GraphPlan.forward_records: no pack, no statistics pass).

Round 8: --dropout P times the step with feature dropout fused into the top-k and the scatter
(maxk_aggregate(..., dropout_p=P)) against the composition a layer with feat_drop ran before
(maxk -> F.dropout -> spgemm, same graph and k) in the same process, the composition twice
(before and after the fused step) so its own spread is known, with each step's peak memory
above the resident tensors, and the dropout top-k / scatter kernels next to the plain ones.

Round 9: --self times the step of a layer with a self term (GraphSAGE, GIN):
x_m, y = maxk_self_aggregate(x, graph, k), backward with upstream gradients for both outputs,
against the composition maxk -> densify -> spgemm (with F.dropout on the [N, k] values under
--dropout) in the same process, the composition before and after the fused step, each step's
peak memory, and the dense top-k / merge scatter kernels next to the plain ones.

Round 10: --edge-weight times the step with a learnable per-edge weight
(maxk_aggregate(x, graph, k, edge_weight=w), w [E] requiring grad) against the constant-weight
step in the same process, the constant step before and after, and separately the passes the
weighted step adds: the effective-value multiply and its backward, the value refresh of the
weighted plan (forward-only, since the backward re-refreshes only after another weighted call),
and the SDDMM edge-gradient kernel.

  python tools/autograd_step.py [--dataset reddit] [--k 16] [--dropout 0.5] [--self]
                                [--edge-weight]
  rocprofv3 --kernel-trace --stats ... -- python tools/autograd_step.py --only-step 20
    (nothing but 20 maxk_aggregate steps: the kernel list of the fused step)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spgemm-gnn_amd"))
import torch  # noqa: E402

import maxk_kernels as mk  # noqa: E402
from maxk_kernels import graphs  # noqa: E402


def timeit(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def host_time(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3 / reps


def peak_bytes(fn):
    """Peak device memory of one call above what is resident before it."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def dropout_report(args, graph, x, g, d, k, step_dropout, step_composed):
    p, dev, n = args.dropout, x.device, x.shape[0]
    t_comp1 = timeit(step_composed)
    t_fused = timeit(step_dropout)
    t_comp2 = timeit(step_composed)
    t_fused2 = timeit(step_dropout)
    t_host = host_time(step_dropout)
    mem_fused, mem_comp = peak_bytes(step_dropout), peak_bytes(step_composed)
    plan = graph.plan(d, k)
    fixed = plan.fwd_fixed
    st = torch.empty(2, dtype=torch.int32, device=dev) if fixed else None
    rec = plan.new_records()
    xd = x.detach()
    if rec is not None:
        def topk(drop):
            return mk.maxk_forward(xd, k, return_index=True, records=rec, return_values=False,
                                   stats=st, dropout=drop)
    else:
        out = plan.new_cbsr()

        def topk(drop):
            return mk.maxk_forward(xd, k, return_index=True, out=out, stats=st, dropout=drop)
    sp_index = topk(None)[1]
    gsp = graphs.features(n, k, seed=99, device=dev)
    seed = 0x9E3779B97F4A7C15
    kern = {
        "topk_ms": timeit(lambda: topk(None)),
        "topk_dropout_ms": timeit(lambda: topk((p, seed))),
        "topk_tables_ms": timeit(lambda: mk.maxk_forward(xd, k, return_index=True)),
        "topk_tables_dropout_ms": timeit(lambda: mk.maxk_forward(xd, k, return_index=True,
                                                                 dropout=(p, seed))),
        "scatter_ms": timeit(lambda: mk.maxk_backward(gsp, sp_index, d)),
        "scatter_dropout_ms": timeit(lambda: mk.maxk_backward(gsp, sp_index, d,
                                                              dropout=(p, seed))),
    }
    kern["topk_ratio"] = kern["topk_dropout_ms"] / kern["topk_ms"]
    kern["topk_tables_ratio"] = kern["topk_tables_dropout_ms"] / kern["topk_tables_ms"]
    kern["scatter_ratio"] = kern["scatter_dropout_ms"] / kern["scatter_ms"]
    info = plan.info()
    print(json.dumps({"dataset": args.dataset, "k": k, "dropout": p,
                      "fwd_layout": info["fwd_layout"], "fwd_fixed": int(fixed),
                      "step_ms_fused_dropout": t_fused, "step_ms_fused_dropout_again": t_fused2,
                      "step_ms_composed": [t_comp1, t_comp2],
                      "fused_not_slower": t_fused <= max(t_comp1, t_comp2),
                      "host_ms_per_step_fused_dropout": t_host,
                      "peak_bytes_fused": mem_fused, "peak_bytes_composed": mem_comp,
                      "peak_bytes_saved": mem_comp - mem_fused, "kernels": kern}), flush=True)


def edge_weight_report(args, graph, x, g, d, k, step_fresh):
    dev, n, e = x.device, x.shape[0], graph.num_edges
    w = (torch.rand(e, device=dev) + 0.5).requires_grad_(True)

    def step_weighted():
        x.grad = None
        w.grad = None
        y = mk.maxk_aggregate(x, graph, k, edge_weight=w)
        y.backward(g)

    t_const1 = timeit(step_fresh)
    t_w = timeit(step_weighted)
    t_const2 = timeit(step_fresh)
    t_w2 = timeit(step_weighted)
    t_host = host_time(step_weighted)
    mem_w, mem_const = peak_bytes(step_weighted), peak_bytes(step_fresh)
    plan = graph.weighted_plan(d, k)
    sp_data, sp_index = mk.maxk_forward(x.detach(), k, return_index=True)
    val = (graph.val * w).detach()
    gval = torch.empty(e, device=dev)
    parts = {
        "refresh_values_ms": timeit(lambda: plan.refresh_values(val)),
        "sddmm_edge_grad_ms": timeit(lambda: mk.spgemm_edge_grad(
            graph.ptr, graph.idx, g, sp_data, sp_index, n, e, k, d, out=gval)),
        "effective_values_mul_ms": timeit(lambda: graph.val * w.detach()),
        "mul_backward_ms": timeit(lambda: gval * graph.val),
    }
    rec = plan.new_records()
    if rec is not None:  # the weighted top-k also writes the plain value table (for the SDDMM)
        xd = x.detach()
        parts["topk_values_table_extra_ms"] = (
            timeit(lambda: mk.maxk_forward(xd, k, return_index=True, records=rec))
            - timeit(lambda: mk.maxk_forward(xd, k, return_index=True, records=rec,
                                             return_values=False)))
    print(json.dumps({"dataset": args.dataset, "k": k, "edge_weight": True,
                      "fwd_layout": plan.info()["fwd_layout"], "fwd_fixed": int(plan.fwd_fixed),
                      "step_ms_edge_weight": t_w, "step_ms_edge_weight_again": t_w2,
                      "step_ms_constant": [t_const1, t_const2],
                      "added_ms": t_w - min(t_const1, t_const2),
                      "host_ms_per_step_edge_weight": t_host,
                      "peak_bytes_edge_weight": mem_w, "peak_bytes_constant": mem_const,
                      "added_parts": parts, "added_parts_sum_ms": sum(parts.values())}),
          flush=True)


def self_report(args, graph, x, g, g_self, d, k, step_self, step_self_composed):
    p, dev, n = args.dropout, x.device, x.shape[0]
    t_comp1 = timeit(step_self_composed)
    t_fused = timeit(step_self)
    t_comp2 = timeit(step_self_composed)
    t_fused2 = timeit(step_self)
    t_host = host_time(step_self)
    mem_fused, mem_comp = peak_bytes(step_self), peak_bytes(step_self_composed)
    plan = graph.plan(d, k)
    fixed = plan.fwd_fixed
    st = torch.empty(2, dtype=torch.int32, device=dev) if fixed else None
    rec = plan.new_records()
    xd = x.detach()
    dense = torch.empty_like(xd)
    seed = 0x9E3779B97F4A7C15
    drop = (p, seed) if p > 0 else None
    if rec is not None:
        def topk(dn):
            return mk.maxk_forward(xd, k, return_index=True, records=rec, return_values=False,
                                   stats=st, dropout=drop, dense=dn)
    else:
        out = plan.new_cbsr()

        def topk(dn):
            return mk.maxk_forward(xd, k, return_index=True, out=out, stats=st, dropout=drop,
                                   dense=dn)
    sp_index = topk(None)[1]
    sp_data = mk.maxk_forward(xd, k, dropout=drop)
    gsp = graphs.features(n, k, seed=99, device=dev)
    idx64 = sp_index.long()
    kern = {
        "topk_ms": timeit(lambda: topk(None)),
        "topk_dense_ms": timeit(lambda: topk(dense)),
        "scatter_ms": timeit(lambda: mk.maxk_backward(gsp, sp_index, d, dropout=drop)),
        "scatter_merge_ms": timeit(lambda: mk.maxk_backward(gsp, sp_index, d, dropout=drop,
                                                            grad_dense=g_self)),
        # the passes of the composition that the two kernels replace
        "densify_ms": timeit(lambda: mk.densify(sp_data, sp_index, d)),
        "densify_grad_gather_add_ms": timeit(lambda: g_self.gather(1, idx64) + gsp),
        "index_long_ms": timeit(lambda: sp_index.long()),
    }
    info = plan.info()
    slower = max(t_comp1, t_comp2)
    print(json.dumps({"dataset": args.dataset, "k": k, "self": True, "dropout": p,
                      "fwd_layout": info["fwd_layout"], "fwd_fixed": int(fixed),
                      "step_ms_self_fused": t_fused, "step_ms_self_fused_again": t_fused2,
                      "step_ms_self_composed": [t_comp1, t_comp2],
                      "fused_not_slower": t_fused <= slower,
                      "speedup_vs_slower_composed": slower / t_fused,
                      "speedup_vs_faster_composed": min(t_comp1, t_comp2) / t_fused,
                      "host_ms_per_step_self_fused": t_host,
                      "peak_bytes_fused": mem_fused, "peak_bytes_composed": mem_comp,
                      "peak_bytes_saved": mem_comp - mem_fused, "kernels": kern}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="reddit")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--only-step", type=int, default=0, metavar="N",
                    help="run N maxk_aggregate steps and nothing else (for a kernel trace)")
    ap.add_argument("--dropout", type=float, default=0.0, metavar="P",
                    help="time the fused-dropout step against maxk -> F.dropout -> spgemm")
    ap.add_argument("--self", dest="self_term", action="store_true",
                    help="time maxk_self_aggregate (dense masked row + aggregation) against "
                         "maxk -> densify -> spgemm")
    ap.add_argument("--edge-weight", dest="edge_weight", action="store_true",
                    help="time the step with a learnable edge_weight against the constant one")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, _ = graphs.DATASETS[args.dataset]
    ptr, idx = graphs.bench_csr(args.dataset, device=dev)
    graph = mk.CSRGraph(ptr, idx, graphs.sage_mean_values(ptr))
    d, k = 256, args.k
    x = graphs.features(n, d, seed=97, device=dev).requires_grad_(True)
    g = graphs.features(n, d, seed=98, device=dev)

    def step():  # x.grad accumulates across steps (no zero_grad), as in a loop without one
        y = mk.maxk_aggregate(x, graph, k)
        y.backward(g)

    def step_fresh():  # optimizer.zero_grad(set_to_none=True) before every step
        x.grad = None
        y = mk.maxk_aggregate(x, graph, k)
        y.backward(g)

    def step_unfused():  # round 5's composition: MaxKFunction -> SpGEMMFunction (the forward
        x.grad = None    # packs / scans the CBSR tables it is handed)
        sd, si = mk.maxk(x, k)
        y = mk.spgemm(sd, si, graph, d)
        y.backward(g)

    p_drop = args.dropout

    def step_dropout():  # dropout inside the top-k and the scatter: seed drawn per step
        x.grad = None
        y = mk.maxk_aggregate(x, graph, k, dropout_p=p_drop)
        y.backward(g)

    def step_composed():  # what a layer with feat_drop > 0 ran before: a mask tensor, a
        x.grad = None     # dropped [N, k] copy, and the forward's pack / statistics pass
        sd, si = mk.maxk(x, k)
        sd = torch.nn.functional.dropout(sd, p_drop, True)
        y = mk.spgemm(sd, si, graph, d)
        y.backward(g)

    g_self = graphs.features(n, d, seed=96, device=dev) if args.self_term else None

    def step_self():  # a layer with a self term: the dense masked row and its aggregation
        x.grad = None
        xm, y = mk.maxk_self_aggregate(x, graph, k, dropout_p=p_drop)
        torch.autograd.backward([xm, y], [g_self, g])

    def step_self_composed():  # what those layers ran before
        x.grad = None
        sd, si = mk.maxk(x, k)
        if p_drop > 0:
            sd = torch.nn.functional.dropout(sd, p_drop, True)
        xm = mk.densify(sd, si, d)
        y = mk.spgemm(sd, si, graph, d)
        torch.autograd.backward([xm, y], [g_self, g])

    if args.only_step:
        for _ in range(args.only_step):
            if args.self_term:
                step_self()
            else:
                step_dropout() if p_drop > 0 else step_fresh()
        torch.cuda.synchronize()
        info = graph.plan(d, k).info()
        print(json.dumps({"dataset": args.dataset, "k": k, "steps": args.only_step,
                          "dropout": p_drop, "self": args.self_term,
                          "fwd_layout": info["fwd_layout"], "fwd_fixed": info["fwd_fixed"],
                          "fwd_split_rows": info["fwd_split_rows"]}), flush=True)
        return
    if args.edge_weight:
        edge_weight_report(args, graph, x, g, d, k, step_fresh)
        return
    if args.self_term:
        self_report(args, graph, x, g, g_self, d, k, step_self, step_self_composed)
        return
    if p_drop > 0:
        dropout_report(args, graph, x, g, d, k, step_dropout, step_composed)
        return
    t_step = timeit(step)
    t_fresh = timeit(step_fresh)
    t_unfused = timeit(step_unfused)
    t_fresh2 = timeit(step_fresh)   # again, after the unfused variant (order effects)
    t_host = host_time(step_fresh)
    mem_fresh = peak_bytes(step_fresh)
    plan = graph.plan(d, k)
    sp_data, sp_index = mk.maxk_forward(x.detach(), k, return_index=True)
    out = torch.empty(n, d, device=dev)
    gsp = torch.empty(n, k, device=dev)
    fixed = plan.fwd_fixed
    st = torch.empty(2, dtype=torch.int32, device=dev) if fixed else None
    st2 = st.view(1, 2) if fixed else None
    rec = plan.new_records()
    if rec is not None:
        def topk_fused():
            return mk.maxk_forward(x.detach(), k, return_index=True, records=rec,
                                   return_values=False, stats=st)

        def fwd_fused():
            return plan.forward_records(rec[0], rec[1], out, stats=st2)
    else:
        rd, ri = plan.new_cbsr()

        def topk_fused():
            return mk.maxk_forward(x.detach(), k, return_index=True, out=(rd, ri), stats=st)

        def fwd_fused():
            return plan.forward(rd, ri, out, stats=st2)
    topk_fused()
    fused = {
        "path": "records" if rec is not None else "tables",
        "topk_stats_layout_ms": timeit(topk_fused),
        "spgemm_fwd_given_stats_ms": timeit(fwd_fused),
    }
    parts = {
        "topk_ms": timeit(lambda: mk.maxk_forward(x.detach(), k, return_index=True)),
        "spgemm_fwd_ms": timeit(lambda: plan.forward(sp_data, sp_index, out)),
        "sspmm_bwd_ms": timeit(lambda: plan.backward(g, sp_index, gsp)),
        "maxk_scatter_ms": timeit(lambda: mk.maxk_backward(gsp, sp_index, d)),
    }
    print(json.dumps({"dataset": args.dataset, "k": k, "fwd_layout": plan.info()["fwd_layout"],
                      "fwd_fixed": int(fixed),
                      "step_ms": t_step, "step_ms_grad_none": t_fresh,
                      "step_ms_grad_none_again": t_fresh2, "step_ms_unfused": t_unfused,
                      "host_ms_per_step": t_host, "peak_bytes_grad_none": mem_fresh,
                      "fused_parts": fused,
                      "parts": parts, "parts_sum_ms": sum(parts.values())}), flush=True)


if __name__ == "__main__":
    main()
