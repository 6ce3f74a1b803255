"""Kernel time and peak memory of the 16-bit CBSR product (ops.cbsr_matmul_16) at D = M = 256 on
Reddit- and ogbn-products-sized row counts, next to two comparators on the same inputs: (i) what
LinearMaxKFunction.backward does without it, weight.float(), ops.cbsr_matmul and .to(dtype); (ii)
what a user has without this library, the dense masked gradient in the 16-bit type (zeros +
scatter_) and gd @ weight in that type through torch. HIP events on the launch stream, warm-up,
medians of --rounds windows of --reps calls, everything alternating inside every round, outputs
preallocated where the call takes them. Peak memory is torch's, above the inputs, of one call of
each path that allocates what it needs. With --steps the record also times one
linear_maxk(fused=True, weight_grad_16=True) forward + backward step with input_grad_16 off and on.
One JSON line per dataset and k, appended to --out; run once per --dtype.

  python tools/cbsr_matmul16_time.py [--datasets reddit,ogbn-products] [--ks 8,16,32,64]
                                     [--dtype bf16|f16] [--steps reddit:16,reddit:64]
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
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def measure(fns, rounds, reps):
    for fn in fns.values():
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


def peak_above(fn):
    """Peak bytes that one call of fn allocates above what is live before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def record(name, k, args, dev):
    dt = DTYPES[args.dtype]
    n, _ = graphs.DATASETS[name]
    w = (graphs.features(D, M, seed=97, device=dev) * 0.06).to(dt)
    # the tables of a real top-k; the values stand for the gradient of the kept values
    _, sel = ops.maxk_forward(graphs.features(n, D, seed=96, device=dev), k, return_index=True)
    grad = graphs.features(n, k, seed=94, device=dev)
    out16 = torch.empty((n, M), dtype=dt, device=dev)
    out32 = torch.empty((n, M), device=dev)
    outd = torch.empty((n, M), dtype=dt, device=dev)
    sel64 = sel.long()  # scatter_'s index type: prepared once, outside the timed call

    def new():
        return ops.cbsr_matmul_16(grad, sel, w, out=out16)

    def upcast():
        return ops.cbsr_matmul(grad, sel, w.float(), out=out32).to(dt)

    def dense():
        gd = torch.zeros((n, D), dtype=dt, device=dev).scatter_(1, sel64, grad.to(dt))
        return torch.mm(gd, w, out=outd)

    fns = {"new_ms": new, "upcast_ms": upcast, "dense_ms": dense}
    rec = {"dataset": name, "n": n, "D": D, "M": M, "k": k, "dtype": args.dtype,
           "rounds": args.rounds, "reps": args.reps, "tile": list(ops.cbsr_matmul_16_tile(D, M))}
    rec.update(measure(fns, args.rounds, args.reps))
    rec["new_tflops"] = 2.0 * n * D * M / rec["new_ms"] / 1e9
    rec["dense_tflops"] = 2.0 * n * D * M / rec["dense_ms"] / 1e9
    rec["new_out_gbs"] = n * M * 2 / rec["new_ms"] / 1e6
    rec["new_over_upcast"] = rec["new_ms"] / rec["upcast_ms"]
    rec["new_over_dense"] = rec["new_ms"] / rec["dense_ms"]
    rec["new_within_upcast"] = bool(rec["new_ms"] <= rec["upcast_ms"])
    rec["new_within_dense"] = bool(rec["new_ms"] <= rec["dense_ms"])
    rec["max_abs_diff_from_upcast"] = float((out16.float() - out32).abs().max())
    rec["new_peak_bytes"] = peak_above(lambda: ops.cbsr_matmul_16(grad, sel, w))
    rec["upcast_peak_bytes"] = peak_above(lambda: ops.cbsr_matmul(grad, sel, w.float()).to(dt))
    rec["dense_peak_bytes"] = peak_above(dense)

    if f"{name}:{k}" in args.steps.split(","):
        # one training step through linear_maxk(fused=True, weight_grad_16=True), flag off and on
        h = graphs.features(n, M, seed=95, device=dev).to(dt)
        b = graphs.features(1, D, seed=98, device=dev)[0].to(dt)
        leaves = [t.clone().requires_grad_(True) for t in (h, w, b)]

        def step(flag):
            for leaf in leaves:
                leaf.grad = None
            data, _ = mk.linear_maxk(*leaves, k, fused=True, weight_grad_16=True,
                                     input_grad_16=flag)
            data.backward(grad)

        rec.update(measure({"step_off_ms": lambda: step(False), "step_on_ms": lambda: step(True)},
                           args.rounds, max(args.reps // 2, 1)))
        rec["step_on_over_off"] = rec["step_on_ms"] / rec["step_off_ms"]
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--ks", default="8,16,32,64")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="bf16")
    ap.add_argument("--steps", default="reddit:16,reddit:64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25",
                                                  "cbsr_matmul16_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cbsr_matmul16_time.py needs a GPU: it measures nothing without one")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.datasets.split(","):
        for k in (int(v) for v in args.ks.split(",")):
            record(name, k, args, dev)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
