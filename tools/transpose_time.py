"""Time of the CSR transposition (maxk_csr_transpose) on the bench graphs, on sampled blocks and on
cluster subgraphs, next to the torch path it replaces on GPU tensors (the private helper
maxk_kernels.autograd._torch_transpose plus the two gathers and casts of transposed_structure) and,
where tools/transpose_hipcub was built, to hipcub's SortPairs over the same key bits (its own
process, random columns, the sort alone). HIP events on the launch stream, warm-up, medians of
--rounds windows of --reps calls (--slow-reps for the torch path), everything alternating inside
every round. GB/s are taken against the compulsory bytes 4 (N + 1) + 4 E read and 4 (NC + 1) + 8 E
written. Peak memory is torch.cuda.max_memory_allocated over transposed_structure() of a fresh
graph object, above what was allocated before it, for the kernel path and for the torch path. One
JSON line per shape, appended to --out.

  python tools/transpose_time.py [--datasets reddit,ogbn-products] [--hipcub tools/transpose_hipcub]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spgemm-gnn_amd"))
import torch  # noqa: E402

import maxk_kernels as mk  # noqa: E402
from maxk_kernels import autograd, graphs, ops  # noqa: E402


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


def torch_structure(ptr, idx, num_cols):
    """transposed_structure() as the torch path computes it."""
    ptr_t, rows, order = autograd._torch_transpose(ptr, idx, num_cols)
    return ptr_t.to(torch.int32), rows[order].to(torch.int32).contiguous(), order


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def one_shape(shape, g, args, emit):
    dev = g.ptr.device
    n, nc, e = g.num_nodes, g._num_cols(), g.num_edges
    out = (torch.empty(nc + 1, dtype=torch.int32, device=dev),
           torch.empty(e, dtype=torch.int32, device=dev),
           torch.empty(e, dtype=torch.int32, device=dev))
    scratch = torch.empty(ops.csr_transpose_scratch_bytes(n, nc, e), dtype=torch.uint8, device=dev)
    ops.csr_transpose(g.ptr, g.idx, None, nc, out=out, scratch=scratch)
    want = torch_structure(g.ptr, g.idx, nc)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    assert torch.equal(out[2], want[2].to(torch.int32))
    del want
    fns = {"kernel_ms": (lambda: ops.csr_transpose(g.ptr, g.idx, None, nc, out=out,
                                                   scratch=scratch), None),
           "kernel_alloc_ms": (lambda: ops.csr_transpose(g.ptr, g.idx, None, nc), None),
           "torch_ms": (lambda: torch_structure(g.ptr, g.idx, nc), args.slow_reps)}
    rec = dict(shape, rows=n, cols=nc, edges=e, digit_bits=list(ops.transpose_digit_bits(nc)),
               scratch_bytes=scratch.numel(), rounds=args.rounds, reps=args.reps,
               slow_reps=args.slow_reps)
    rec.update(measure(fns, args.rounds, args.reps))
    model = 4 * (n + 1) + 4 * e + 4 * (nc + 1) + 8 * e
    rec.update(model_bytes=model, kernel_gbps=model / rec["kernel_ms"] / 1e6,
               torch_vs_kernel=rec["torch_ms"] / rec["kernel_ms"])
    del out, scratch, fns

    def fresh():
        return type(g)(**{f: getattr(g, f) for f in g.__dataclass_fields__ if f != "_values"})

    rec["kernel_peak_bytes"] = peak_bytes(lambda: fresh().transposed_structure())
    rec["torch_peak_bytes"] = peak_bytes(lambda: torch_structure(g.ptr, g.idx, nc))
    if args.hipcub and os.path.exists(args.hipcub) and e > 0:
        run = subprocess.run([args.hipcub, str(e), str(max(nc, 1)), str(args.rounds),
                              str(args.reps)], capture_output=True, text=True, timeout=300)
        if run.returncode == 0:
            rec.update(json.loads(run.stdout.strip().splitlines()[-1]))
            rec["hipcub_vs_kernel"] = rec["hipcub_ms"] / rec["kernel_ms"]
        else:
            rec["hipcub_error"] = run.stderr.strip()[-200:]
    emit(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--seeds", default="65536,1024")
    ap.add_argument("--fanouts", default="10,25")
    ap.add_argument("--parts", default="8,64")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-reps", type=int, default=3, help="calls per window of the torch path")
    ap.add_argument("--hipcub", default=os.path.join(ROOT, "tools", "transpose_hipcub"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "transpose_time.jsonl"))
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
        one_shape({"dataset": name, "shape": "full graph"}, graph, args, emit)
        gen = torch.Generator().manual_seed(3)
        for s in [int(v) for v in args.seeds.split(",") if v]:
            seeds = torch.randperm(n_nodes, generator=gen)[:s].to(torch.int32).to(dev)
            for fanout in [int(v) for v in args.fanouts.split(",") if v]:
                block = mk.to_block(graph, seeds, fanout, 11)
                one_shape({"dataset": name, "shape": f"block, {s} seeds, fanout {fanout}"}, block,
                          args, emit)
                del block
        for parts in [int(v) for v in args.parts.split(",") if v]:
            loader = mk.ClusterLoader(graph, parts, seed=0)
            sub = mk.node_subgraph(graph, loader._members[0])
            one_shape({"dataset": name, "shape": f"subgraph, 1 of {parts} parts"}, sub, args, emit)
            del loader, sub
        del graph, ptr, idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
