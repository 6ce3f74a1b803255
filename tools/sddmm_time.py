"""Kernel time of the SDDMM edge-gradient (maxk_sddmm_edge_grad) on the bench graphs, next to the
same process's SpGEMM forward and SSpMM backward (the same gather volume per edge). HIP events
on the launch stream, warm-up, the median of --rounds windows of --reps launches, the compared
kernels alternating inside every round. One JSON line per (dataset, k).

  python tools/sddmm_time.py [--datasets reddit,ogbn-products] [--ks 8,16,32,64] [--rounds 5]
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


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit")
    ap.add_argument("--ks", default="8,16,32,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    d = 256
    for name in args.datasets.split(","):
        n, _ = graphs.DATASETS[name]
        ptr, idx = graphs.bench_csr(name, device=dev)
        e = idx.numel()
        graph = mk.CSRGraph(ptr, idx, graphs.sage_mean_values(ptr))
        x = graphs.features(n, d, seed=97, device=dev)
        g = graphs.features(n, d, seed=98, device=dev)
        out = torch.empty(n, d, device=dev)
        gval = torch.empty(e, device=dev)
        for k in [int(s) for s in args.ks.split(",")]:
            plan = graph.plan(d, k)
            sp_data, sp_index = mk.maxk_forward(x, k, return_index=True)
            gsp = torch.empty(n, k, device=dev)
            fns = {
                "sddmm_ms": lambda: ops.spgemm_edge_grad(ptr, idx, g, sp_data, sp_index, n, e, k,
                                                         d, out=gval),
                "spgemm_fwd_ms": lambda: plan.forward(sp_data, sp_index, out),
                "sspmm_bwd_ms": lambda: plan.backward(g, sp_index, gsp),
            }
            for fn in fns.values():   # warm-up: code objects, workspaces
                fn()
                fn()
            torch.cuda.synchronize()
            times = {key: [] for key in fns}
            for _ in range(args.rounds):
                for key, fn in fns.items():
                    times[key].append(window(fn, args.reps))
            rec = {"dataset": name, "n": n, "edges": e, "d": d, "k": k,
                   "edges_per_row": e / n, "rounds": args.rounds, "reps": args.reps}
            for key, ts in times.items():
                rec[key] = statistics.median(ts)
                rec[key.replace("_ms", "_min_max_ms")] = [min(ts), max(ts)]
            rec["sddmm_over_sspmm_bwd"] = rec["sddmm_ms"] / rec["sspmm_bwd_ms"]
            print(json.dumps(rec), flush=True)
        del graph, plan
        ops.clear_plan_cache()


if __name__ == "__main__":
    main()
