"""Kernel time of the edge softmax (maxk_edge_softmax_forward / _backward) on the bench graphs,
next to the same process's torch composition (scatter_reduce(amax), gather, subtract, exp,
index_add, gather, divide; its backward is autograd's). HIP events on the launch stream,
warm-up, the median of --rounds windows of --reps launches, the compared calls alternating inside
every round. Bytes per second are against the byte bound of one read and one write per edge plus
ptr: 8 E + 4 N forward, 12 E + 4 N backward. Also timed alone: the graph's longest row (one
work-group of the hub regime) and the sub-graph of all rows above the upper regime limit.
One JSON line per dataset, appended to --out.

  python tools/edge_softmax_time.py [--datasets reddit,ogbn-products] [--rounds 7] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spgemm-gnn_amd"))
import torch  # noqa: E402

from maxk_kernels import graphs, ops  # noqa: E402


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def torch_softmax(x, rows, n):
    m = torch.full((n,), float("-inf"), device=x.device).scatter_reduce(0, rows, x, "amax")
    p = (x - m[rows]).exp()
    s = torch.zeros(n, device=x.device).index_add_(0, rows, p)
    return p / s[rows]


def measure(fns, rounds, reps):
    for fn in fns.values():   # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {key: [] for key in fns}
    for _ in range(rounds):
        for key, fn in fns.items():
            times[key].append(window(fn, reps))
    rec = {}
    for key, ts in times.items():
        rec[key] = statistics.median(ts)
        rec[key.replace("_ms", "_min_max_ms")] = [min(ts), max(ts)]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "edge_softmax.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    limits = ops.edge_softmax_row_limits()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.datasets.split(","):
        n, _ = graphs.DATASETS[name]
        ptr, idx = graphs.bench_csr(name, device=dev)
        e = idx.numel()
        del idx
        deg = graphs.row_degrees(ptr)
        rows = torch.repeat_interleave(torch.arange(n, device=dev), deg, output_size=e)
        x = graphs.features(e, 1, seed=97, device=dev).reshape(e)
        g = graphs.features(e, 1, seed=98, device=dev).reshape(e)
        y, gx = torch.empty(e, device=dev), torch.empty(e, device=dev)
        ops.edge_softmax(ptr, x, out=y)
        xt = x.clone().requires_grad_(True)
        state = {}

        def torch_fwd():
            state["y"] = torch_softmax(xt, rows, n)

        def torch_bwd():
            xt.grad = None
            state["y"].backward(g, retain_graph=True)

        torch_fwd()
        rec = {"dataset": name, "n": n, "edges": e, "edges_per_row": e / n,
               "longest_row": int(deg.max()), "row_limits": list(limits),
               "rounds": args.rounds, "reps": args.reps,
               "max_abs_diff_vs_torch": float((state["y"].detach() - y).abs().max())}
        rec.update(measure({
            "fwd_ms": lambda: ops.edge_softmax(ptr, x, out=y),
            "torch_fwd_ms": torch_fwd,
            "bwd_ms": lambda: ops.edge_softmax_backward(ptr, y, g, out=gx),
            "torch_bwd_ms": torch_bwd,
        }, args.rounds, args.reps))
        state.clear()
        fb, bb = 8 * e + 4 * n, 12 * e + 4 * n
        rec.update(fwd_bound_bytes=fb, bwd_bound_bytes=bb,
                   fwd_tb_per_s=fb / rec["fwd_ms"] * 1e-9, bwd_tb_per_s=bb / rec["bwd_ms"] * 1e-9,
                   fwd_speedup_vs_torch=rec["torch_fwd_ms"] / rec["fwd_ms"],
                   bwd_speedup_vs_torch=rec["torch_bwd_ms"] / rec["bwd_ms"])
        # the hub regime alone: the longest row as a one-row graph, and every row above the
        # upper limit as a graph of its own (their edges gathered into one array)
        r = int(deg.argmax())
        b, m = int(ptr[r]), int(deg[r])
        p1 = torch.tensor([0, m], dtype=torch.int32, device=dev)
        x1, g1 = x[b:b + m].clone(), g[b:b + m].clone()
        y1, gx1 = torch.empty(m, device=dev), torch.empty(m, device=dev)
        one = measure({"longest_row_fwd_ms": lambda: ops.edge_softmax(p1, x1, out=y1),
                       "longest_row_bwd_ms": lambda: ops.edge_softmax_backward(p1, y1, g1, out=gx1)},
                      args.rounds, args.reps)
        rec.update(one, longest_row_regime=sum(m > L for L in limits))
        hub = deg > limits[-1]
        rec["hub_rows"], rec["hub_edges"] = int(hub.sum()), int(deg[hub].sum())
        if rec["hub_rows"]:
            ph = torch.zeros(rec["hub_rows"] + 1, dtype=torch.int64, device=dev)
            ph[1:] = torch.cumsum(deg[hub], 0)
            ph = ph.to(torch.int32)
            sel = hub[rows]
            xh, gh = x[sel].contiguous(), g[sel].contiguous()
            yh, gxh = torch.empty_like(xh), torch.empty_like(xh)
            rec.update(measure({
                "hub_rows_fwd_ms": lambda: ops.edge_softmax(ph, xh, out=yh),
                "hub_rows_bwd_ms": lambda: ops.edge_softmax_backward(ph, yh, gh, out=gxh),
            }, args.rounds, args.reps))
            rec["hub_share_of_fwd"] = rec["hub_rows_fwd_ms"] / rec["fwd_ms"]
            rec["hub_share_of_bwd"] = rec["hub_rows_bwd_ms"] / rec["bwd_ms"]
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del rows, x, g, y, gx, xt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
