"""Time of the induced-subgraph extraction on the bench graphs, and of cluster mini-batches built
on it: maxk_induced_subgraph_count and _fill for one cluster batch of random_partition, next to a
torch restatement of the same extraction on the same device (a node mask gathered over the
selected rows' edges, repeat_interleave, a boolean select, a cumulative sum, a relabel gather: the
same three outputs), the plan build of that subgraph, and a MaxKSAGE (mean) epoch over
ClusterLoader in three forms: cached (the second epoch onwards), uncached (every subgraph, plan
and transposed structure built again), and the sum of the batches' layer steps alone (subgraphs
and gathered features prepared), beside one full-graph step. HIP events on the launch stream,
warm-up, medians of --rounds windows of --reps calls, everything alternating inside every round.
The extraction's bytes per second are taken against 4 (S + sum n) + 4 N + 8 M: nodes and the
selected rows' idx read, one int32 mark per node written, out_col and out_eid written. One JSON
line per (dataset, parts), appended to --out.

  python tools/subgraph_time.py [--datasets reddit,ogbn-products] [--parts 8,64]
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

D, K = 256, 16


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
    for fn, _ in fns.values():
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


def torch_subgraph(ptr64, idx, nodes64, num_nodes):
    """The extraction's three outputs from tensor ops."""
    dev = idx.device
    s = nodes64.numel()
    local = torch.full((num_nodes,), -1, dtype=torch.int64, device=dev)
    local[nodes64] = torch.arange(s, device=dev)
    start = ptr64[nodes64]
    n = ptr64[nodes64 + 1] - start
    seg = torch.repeat_interleave(torch.arange(s, device=dev), n)
    first = torch.cumsum(n, 0) - n
    e = start[seg] + (torch.arange(seg.numel(), device=dev) - first[seg])
    loc = local[idx[e].long()]
    keep = loc >= 0
    out_ptr = torch.zeros(s + 1, dtype=torch.int64, device=dev)
    out_ptr[1:] = torch.cumsum(torch.bincount(seg[keep], minlength=s), 0)
    return out_ptr.to(torch.int32), loc[keep].to(torch.int32), e[keep].to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--parts", default="8,64")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-reps", type=int, default=3,
                    help="calls per window of the torch restatement and the plan build")
    ap.add_argument("--epoch-rounds", type=int, default=3, help="windows of one epoch each")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "subgraph_time.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    for name in [v for v in args.datasets.split(",") if v]:
        n_nodes, _ = graphs.DATASETS[name]
        ptr, idx = graphs.bench_csr(name, device=dev)
        graph = mk.CSRGraph(ptr, idx)
        ptr64 = graph.ptr.long()
        feats = graphs.features(n_nodes, D, seed=95, device=dev)
        torch.manual_seed(17)
        model = mk.MaxKSAGE(D, D, 2, 47, maxk=K, feat_drop=0.0).to(dev)

        def step(g, x):
            model.zero_grad(set_to_none=True)
            model(g, x).square().mean().backward()

        for parts in [int(v) for v in args.parts.split(",")]:
            loader = mk.ClusterLoader(graph, parts, seed=0)
            nodes = loader._members[0]
            nodes64 = nodes.long()
            s = nodes.numel()
            sum_n = int((ptr64[nodes64 + 1] - ptr64[nodes64]).sum())
            out = (torch.empty(s + 1, dtype=torch.int32, device=dev),
                   torch.empty(3, dtype=torch.int32, device=dev))
            scratch = torch.empty(ops.induced_subgraph_scratch_bytes(n_nodes, s),
                                  dtype=torch.uint8, device=dev)
            ops.induced_subgraph_count(graph.ptr, graph.idx, nodes, out=out, scratch=scratch)
            m, distinct, stray = out[1].tolist()
            assert distinct == s and stray == 0
            fout = (torch.empty(m, dtype=torch.int32, device=dev),
                    torch.empty(m, dtype=torch.int32, device=dev))
            ops.induced_subgraph_fill(graph.ptr, graph.idx, nodes, out[0], out=fout,
                                      scratch=scratch)
            want = torch_subgraph(ptr64, graph.idx, nodes64, n_nodes)
            assert torch.equal(want[0], out[0]) and torch.equal(want[1], fout[0])
            assert torch.equal(want[2], fout[1])
            sub = mk.node_subgraph(graph, nodes).with_values("mean")

            def plan_build():
                ops.GraphPlan(sub.ptr, sub.idx, sub.val, sub.num_nodes, sub.num_edges, D, K)

            subs = list(loader)                     # the first epoch builds and keeps them
            xs = [feats[g.node_ids.long()] for g in subs]
            for g, x in zip(subs, xs):
                step(g, x)                          # plans and transposed structures exist

            def cached_epoch():
                for g in loader:
                    step(g, feats[g.node_ids.long()])

            # built once, outside the timed windows: the constructor's host work (a sort of the
            # part ids, P copies to the device) belongs to neither epoch
            uncached = mk.ClusterLoader(graph, loader.parts, cache=False)

            def uncached_epoch():
                for g in uncached:
                    step(g, feats[g.node_ids.long()])

            def steps_only():
                for g, x in zip(subs, xs):
                    step(g, x)

            slow = args.slow_reps
            fns = {
                "count_ms": (lambda: ops.induced_subgraph_count(
                    graph.ptr, graph.idx, nodes, out=out, scratch=scratch), None),
                "fill_ms": (lambda: ops.induced_subgraph_fill(
                    graph.ptr, graph.idx, nodes, out[0], out=fout, scratch=scratch), None),
                "torch_subgraph_ms": (lambda: torch_subgraph(ptr64, graph.idx, nodes64, n_nodes),
                                      slow),
                "node_subgraph_ms": (lambda: mk.node_subgraph(graph, nodes), slow),
                "plan_build_ms": (plan_build, slow),
            }
            rec = {"dataset": name, "n": n_nodes, "edges": graph.num_edges, "parts": parts,
                   "selected": s, "selected_rows_edges": sum_n, "kept_edges": m, "D": D, "k": K,
                   "rounds": args.rounds, "reps": args.reps, "slow_reps": slow,
                   "epoch_rounds": args.epoch_rounds,
                   "epoch_kept_edges": sum(g.num_edges for g in subs)}
            rec.update(measure(fns, args.rounds, args.reps))
            epochs = {"cached_epoch_ms": (cached_epoch, 1), "steps_only_ms": (steps_only, 1),
                      "uncached_epoch_ms": (uncached_epoch, 1),
                      "full_graph_step_ms": (lambda: step(graph, feats), 1)}
            rec.update(measure(epochs, args.epoch_rounds, 1))
            model_bytes = 4 * (s + sum_n) + 4 * n_nodes + 8 * m
            rec.update(
                extract_ms=rec["count_ms"] + rec["fill_ms"],
                extract_model_bytes=model_bytes,
                extract_gbps=model_bytes / (rec["count_ms"] + rec["fill_ms"]) / 1e6,
                torch_vs_extract=rec["torch_subgraph_ms"] / (rec["count_ms"] + rec["fill_ms"]),
                cached_vs_steps=rec["cached_epoch_ms"] / rec["steps_only_ms"],
                uncached_vs_cached=rec["uncached_epoch_ms"] / rec["cached_epoch_ms"])
            emit(rec)
            del loader, uncached, subs, xs, sub, fns, epochs
            mk.clear_plan_cache()
            torch.cuda.empty_cache()
        del graph, feats, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
