"""Kernel time of the max aggregation on the bench graphs: maxk_max_aggregate_forward with and
without arg_*, its backward, and the pool layer step (forward plus backward through autograd)
next to the mean layer step. For context, timed in the same alternation and reported without a
bar: the plan SpGEMM forward and SSpMM backward at the same k, and heads_aggregate forward and
backward at H = 1, the nearest plan-less kernel (the same gathers plus alpha). HIP events on the
launch stream, warm-up, medians of --rounds windows of --reps calls, everything alternating
inside every round. The forward's bytes per second are taken against its compulsory traffic,
9 N D + 4 E + 5 k N_cols bytes (out, arg_edge and arg_slot written once, idx and the tables read
once).

--torch-datasets: the torch composition (gather of the [E, D] messages, scatter_reduce(amax)
and autograd's backward) on the first of these graphs whose messages fit in memory, next to the
kernels on the same graph. One JSON line per dataset and k, appended to --out.

  python tools/max_aggregate_time.py [--datasets reddit,ogbn-products] [--ks 16,32]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spgemm-gnn_amd"))
import torch  # noqa: E402

import maxk_kernels as mk  # noqa: E402
from maxk_kernels import graphs, ops  # noqa: E402

D = 256


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def measure(fns, rounds, reps):
    """fns: key -> (fn, reps or None). Medians and [min, max] of `rounds` windows per key."""
    for fn, _ in fns.values():   # warm-up: code objects, allocator, plans
        fn()
        fn()
    torch.cuda.synchronize()
    times = {key: [] for key in fns}
    for _ in range(rounds):
        for key, (fn, r) in fns.items():
            times[key].append(window(fn, r or reps))
    rec = {}
    for key, ts in times.items():
        rec[key] = statistics.median(ts)
        rec[key.replace("_ms", "_min_max_ms")] = [min(ts), max(ts)]
    return rec


def kernel_fns(graph, x, gout, k):
    """The timed calls on `graph` at k: the max kernels, the plan kernels, heads at H = 1."""
    n, e = graph.num_nodes, graph.num_edges
    ptr_t, idx_t, _ = graph.transposed_structure()
    order = graph.transposed_order()
    sp_data, sp_index = ops.maxk_forward(x, k, return_index=True)
    _, ae, sl = ops.max_aggregate_forward(graph.ptr, graph.idx, sp_data, sp_index, D)
    alpha = torch.ones((1, e), device=x.device)
    plan = graph.plan(D, k)
    return {
        "max_fwd_ms": (lambda: ops.max_aggregate_forward(graph.ptr, graph.idx, sp_data, sp_index,
                                                         D), None),
        "max_fwd_noarg_ms": (lambda: ops.max_aggregate_forward(graph.ptr, graph.idx, sp_data,
                                                               sp_index, D, False), None),
        "max_bwd_ms": (lambda: ops.max_aggregate_backward(ptr_t, idx_t, order, gout, ae, sl,
                                                          sp_index), None),
        "heads1_fwd_ms": (lambda: ops.heads_aggregate(graph.ptr, graph.idx, alpha, sp_data,
                                                      sp_index, D), None),
        "heads1_bwd_ms": (lambda: ops.heads_aggregate_backward(
            ptr_t, idx_t, order, alpha, gout, sp_data, sp_index, need_alpha=False), None),
        "plan_spgemm_fwd_ms": (lambda: plan.forward(sp_data, sp_index), None),
        "plan_sspmm_bwd_ms": (lambda: plan.backward(gout, sp_index), None),
    }, (sp_data, sp_index)


def layer_fns(graph, x, gout, k):
    fns = {}
    for agg in ("mean", "pool"):
        torch.manual_seed(16)
        layer = mk.MaxKSAGEConv(D, D, agg, maxk=k).to(x.device)
        feat = x.clone().requires_grad_(True)

        def step(layer=layer, feat=feat):
            feat.grad = None
            layer.zero_grad(set_to_none=True)
            layer(graph, feat).backward(gout)

        fns[f"{agg}_layer_step_ms"] = (step, None)
    return fns


def torch_fns(graph, tables, gout):
    """gather -> scatter_reduce(amax) -> autograd's backward on the densified tables."""
    sp_data, sp_index = tables
    X = mk.densify(sp_data, sp_index, D).requires_grad_(True)
    rows = graph.edge_rows()[:, None].expand(-1, D)
    cols = graph.idx.long()

    def fwd():
        out = torch.zeros((graph.num_nodes, D), device=X.device)
        return out.scatter_reduce(0, rows, X[cols], "amax", include_self=False)

    def step():
        X.grad = None
        fwd().backward(gout)

    def fwd_only():
        with torch.no_grad():
            fwd()

    return {"torch_fwd_ms": (fwd_only, None), "torch_step_ms": (step, None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--torch-datasets", default="ogbn-proteins,yelp")
    ap.add_argument("--ks", default="16,32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "max_aggregate.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    ks = [int(v) for v in args.ks.split(",")]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    def load(name):
        n, _ = graphs.DATASETS[name]
        ptr, idx = graphs.bench_csr(name, device=dev)
        return (mk.CSRGraph(ptr, idx), graphs.features(n, D, seed=95, device=dev),
                graphs.features(n, D, seed=96, device=dev))

    for name in [v for v in args.datasets.split(",") if v]:
        graph, x, gout = load(name)
        n, e = graph.num_nodes, graph.num_edges
        for k in ks:
            fns, _ = kernel_fns(graph, x, gout, k)
            fns.update(layer_fns(graph, x, gout, k))
            rec = {"dataset": name, "n": n, "edges": e, "D": D, "k": k, "rounds": args.rounds,
                   "reps": args.reps}
            rec.update(measure(fns, args.rounds, args.reps))
            fwd_bytes = 9 * n * D + 4 * e + 5 * k * n
            rec.update(
                fwd_model_bytes=fwd_bytes,
                max_fwd_gbps=fwd_bytes / rec["max_fwd_ms"] / 1e6,
                max_fwd_vs_heads1_fwd=rec["max_fwd_ms"] / rec["heads1_fwd_ms"],
                max_bwd_vs_heads1_bwd=rec["max_bwd_ms"] / rec["heads1_bwd_ms"],
                max_fwd_vs_plan_fwd=rec["max_fwd_ms"] / rec["plan_spgemm_fwd_ms"],
                pool_vs_mean_layer_step=rec["pool_layer_step_ms"] / rec["mean_layer_step_ms"])
            emit(rec)
            fns = None
            torch.cuda.empty_cache()
        del graph, x, gout
        torch.cuda.empty_cache()

    for name in [v for v in args.torch_datasets.split(",") if v]:
        graph, x, gout = load(name)
        n, e = graph.num_nodes, graph.num_edges
        k = ks[0]
        fns, tables = kernel_fns(graph, x, gout, k)
        fns = {key: fns[key] for key in ("max_fwd_ms", "max_fwd_noarg_ms", "max_bwd_ms")}
        try:
            comp = torch_fns(graph, tables, gout)
            for fn, _ in comp.values():
                fn()
            torch.cuda.synchronize()
        except torch.OutOfMemoryError:
            emit({"dataset": name, "n": n, "edges": e, "D": D, "k": k,
                  "torch_composition": "out of memory", "message_bytes": 4 * e * D})
            del graph, x, gout, fns
            comp = None
            torch.cuda.empty_cache()
            continue
        fns.update({key: (fn, args.torch_reps) for key, (fn, _) in comp.items()})
        rec = {"dataset": name, "n": n, "edges": e, "D": D, "k": k, "rounds": args.rounds,
               "reps": args.reps, "torch_reps": args.torch_reps, "message_bytes": 4 * e * D}
        rec.update(measure(fns, args.rounds, args.reps))
        rec.update(torch_fwd_vs_max_fwd=rec["torch_fwd_ms"] / rec["max_fwd_noarg_ms"],
                   torch_step_vs_max_step=rec["torch_step_ms"] /
                   (rec["max_fwd_ms"] + rec["max_bwd_ms"]))
        emit(rec)
        break


if __name__ == "__main__":
    main()
