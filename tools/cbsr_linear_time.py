"""Kernel time of the CBSR-times-table products (ops.cbsr_matmul, cbsr_sampled_matmul,
cbsr_weight_grad) at D = M = 256 on Reddit- and ogbn-products-sized row counts, each next to the
dense path it replaces, in the same process:
  * (A) against x_m @ W.T on the dense masked row, and, as the backward of a linear in front of a
    MaxK, against maxk_scatter_backward + grad_x @ W;
  * (C) with its sums against grad_x.T @ h plus the column sum;
  * (B) + (C) against the two GEMMs of torch's backward of the dense self term;
  * the MaxKSAGEConv forward + backward step with sparse_linear on and off (on the dataset's graph).
Each kernel's bytes per second count its one [N, M] stream plus the tables. HIP events on the
launch stream, warm-up, medians of --rounds windows of --reps calls, everything alternating inside
every round. One JSON line per dataset and k, appended to --out.

  python tools/cbsr_linear_time.py [--datasets reddit,ogbn-products] [--ks 8,16,32,64]
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

D = M = 256


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


def record(name, k, args, dev):
    n, _ = graphs.DATASETS[name]
    x = graphs.features(n, D, seed=95, device=dev)
    g = graphs.features(n, M, seed=96, device=dev)
    w = graphs.features(M, D, seed=97, device=dev) * 0.06      # nn.Linear's [out, in]
    wt = w.t().contiguous()
    v, s = ops.maxk_forward(x, k, return_index=True)
    x_m = mk.densify(v, s, D)
    gsp = graphs.features(n, k, seed=98, device=dev)
    out_nm, grad_x, dense_nm = (torch.empty((n, M), device=dev) for _ in range(3))
    out_nk = torch.empty((n, k), device=dev)
    d_t, d_sum, dense_t = torch.empty((D, M), device=dev), torch.empty(D, device=dev), \
        torch.empty((D, M), device=dev)
    scratch = [torch.empty(ops.cbsr_linear_scratch_bytes(op, n, D, k, M), dtype=torch.uint8,
                           device=dev) for op in (1, 2)]

    def sampled():
        ops.cbsr_sampled_matmul(g, s, wt, out=out_nk, scratch=scratch[0])

    def weight_grad():
        ops.cbsr_weight_grad(v, s, g, D, with_sum=True, out=(d_t, d_sum), scratch=scratch[1])

    def dense_linear_bwd_input():
        torch.matmul(ops.maxk_backward(gsp, s, dim_origin=D), w, out=dense_nm)

    def dense_weight_grad():
        torch.matmul(x_m.t(), g, out=dense_t)
        x_m.sum(0)

    def dense_self_bwd():
        torch.matmul(g, w, out=dense_nm)
        torch.matmul(g.t(), x_m, out=dense_t)

    def sparse_self_bwd():
        sampled()
        weight_grad()

    fns = {
        "matmul_ms": (lambda: ops.cbsr_matmul(v, s, wt, out=out_nm), None),
        "dense_matmul_ms": (lambda: torch.matmul(x_m, wt, out=dense_nm), None),
        "dense_scatter_matmul_ms": (dense_linear_bwd_input, None),
        "sampled_ms": (sampled, None),
        "weight_grad_ms": (weight_grad, None),
        "dense_weight_grad_ms": (dense_weight_grad, None),
        "sparse_self_bwd_ms": (sparse_self_bwd, None),
        "dense_self_bwd_ms": (dense_self_bwd, None),
    }
    if not args.no_layer:
        ptr, idx = graphs.bench_csr(name, device=dev)
        graph = mk.CSRGraph(ptr, idx)
        feat = x.clone().requires_grad_(True)
        for flag in (False, True):
            torch.manual_seed(1)
            layer = mk.MaxKSAGEConv(D, M, "mean", maxk=k, sparse_linear=flag).to(dev)

            def step(layer=layer):
                feat.grad = None
                layer.zero_grad(set_to_none=True)
                layer(graph, feat).backward(g)

            fns["sage_step_sparse_ms" if flag else "sage_step_dense_ms"] = (step, args.step_reps)
    rec = {"dataset": name, "n": n, "D": D, "M": M, "k": k, "rounds": args.rounds,
           "reps": args.reps, "panel": list(ops.cbsr_linear_panel(D, M))}
    rec.update(measure(fns, args.rounds, args.reps))
    stream, tables = 4 * n * M, 5 * n * k + 4 * D * M
    for key, extra in (("matmul", 0), ("sampled", -n * k), ("weight_grad", 0)):
        rec[key + "_gb_per_s"] = (stream + tables + extra) / rec[key + "_ms"] / 1e6
    rec["stream_gb"] = stream / 1e9
    for new, old in (("matmul_ms", "dense_matmul_ms"), ("matmul_ms", "dense_scatter_matmul_ms"),
                     ("weight_grad_ms", "dense_weight_grad_ms"),
                     ("sparse_self_bwd_ms", "dense_self_bwd_ms"),
                     ("sage_step_sparse_ms", "sage_step_dense_ms")):
        if new in rec and old in rec:
            rec[old.replace("_ms", "") + "_over_" + new.replace("_ms", "")] = rec[old] / rec[new]
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--ks", default="8,16,32,64")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--no-layer", action="store_true", help="skip the MaxKSAGEConv step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21",
                                                  "cbsr_linear_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cbsr_linear_time.py needs a GPU: it measures nothing without one")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.datasets.split(","):
        for k in (int(v) for v in args.ks.split(",")):
            record(name, k, args, dev)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
