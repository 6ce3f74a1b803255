"""Kernel time and peak memory of the fused linear + MaxK (ops.linear_topk) at D = D_in = 256 on
Reddit- and ogbn-products-sized row counts, next to the composition it replaces on the same inputs:
F.linear into a dense [N, D] tensor, then ops.maxk_forward on it. The two parts of the composition
are also timed alone, so that the expectation `fused <= GEMM + top-k` can be read off one record.
HIP events on the launch stream, warm-up, medians of --rounds windows of --reps calls, everything
alternating inside every round, outputs preallocated. Peak memory is torch's, above the inputs, of
one call of each path that allocates its own outputs. One JSON line per dataset and k, appended to
--out.

With --dtype bf16 or f16 the fused call is the 16-bit kernel on h and W rounded to that type, timed
against (1) the composition a user has without it: F.linear in the same type into a 16-bit [N, D],
.float(), ops.maxk_forward; (2) the f32 ops.linear_topk; (3) f32 rocBLAS + top-k; the record also
holds the share of rows whose selectors differ from the f32 fused path's.

  python tools/linear_topk_time.py [--datasets reddit,ogbn-products] [--ks 8,16,32,64]
                                   [--dtype f32|bf16|f16]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spgemm-gnn_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from maxk_kernels import graphs, ops  # noqa: E402

D = D_IN = 256
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


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
    n, _ = graphs.DATASETS[name]
    h = graphs.features(n, D_IN, seed=95, device=dev)
    w = graphs.features(D, D_IN, seed=97, device=dev) * 0.06      # nn.Linear's [out, in]
    b = graphs.features(1, D, seed=98, device=dev)[0].contiguous()
    y = torch.empty((n, D), device=dev)
    tables = [(torch.empty((n, k), device=dev), torch.empty((n, k), dtype=torch.uint8, device=dev))
              for _ in range(2)]

    def gemm():
        torch.addmm(b, h, w.t(), out=y)

    def topk():
        ops.maxk_forward(y, k, return_index=True, out=tables[0])

    def composition():
        gemm()
        topk()

    fns = {"fused_ms": lambda: ops.linear_topk(h, w, b, k, out=tables[1]),
           "composition_ms": composition, "gemm_ms": gemm, "topk_ms": topk}
    rec = {"dataset": name, "n": n, "D": D, "D_in": D_IN, "k": k, "rounds": args.rounds,
           "reps": args.reps, "tile": list(ops.linear_topk_tile(D))}
    rec.update(measure(fns, args.rounds, args.reps))
    rec["tables_equal"] = bool(torch.equal(tables[0][1], tables[1][1]))
    rec["values_max_abs_diff"] = float((tables[0][0] - tables[1][0]).abs().max())
    rec["fused_tflops"] = 2.0 * n * D * D_IN / rec["fused_ms"] / 1e9
    rec["gemm_tflops"] = 2.0 * n * D * D_IN / rec["gemm_ms"] / 1e9
    rec["fused_over_composition"] = rec["fused_ms"] / rec["composition_ms"]
    rec["fused_within_gemm_plus_topk"] = bool(rec["fused_ms"] <= rec["gemm_ms"] + rec["topk_ms"])
    rec["fused_peak_bytes"] = peak_above(lambda: ops.linear_topk(h, w, b, k))
    rec["composition_peak_bytes"] = peak_above(
        lambda: ops.maxk_forward(F.linear(h, w, b), k, return_index=True))
    rec["dense_preactivation_bytes"] = 4 * n * D
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def record16(name, k, args, dev):
    dt = DTYPES[args.dtype]
    n, _ = graphs.DATASETS[name]
    h = graphs.features(n, D_IN, seed=95, device=dev)
    w = graphs.features(D, D_IN, seed=97, device=dev) * 0.06
    b = graphs.features(1, D, seed=98, device=dev)[0].contiguous()
    h16, w16, b16 = h.to(dt), w.to(dt), b.to(dt)
    y, y16 = torch.empty((n, D), device=dev), torch.empty((n, D), dtype=dt, device=dev)
    tables = [(torch.empty((n, k), device=dev), torch.empty((n, k), dtype=torch.uint8, device=dev))
              for _ in range(4)]

    def composition16():
        torch.addmm(b16, h16, w16.t(), out=y16)
        y.copy_(y16)
        ops.maxk_forward(y, k, return_index=True, out=tables[1])

    def composition32():
        torch.addmm(b, h, w.t(), out=y)
        ops.maxk_forward(y, k, return_index=True, out=tables[3])

    fns = {"fused16_ms": lambda: ops.linear_topk(h16, w16, b, k, out=tables[0]),
           "composition16_ms": composition16,
           "fused32_ms": lambda: ops.linear_topk(h, w, b, k, out=tables[2]),
           "composition32_ms": composition32}
    rec = {"dataset": name, "n": n, "D": D, "D_in": D_IN, "k": k, "dtype": args.dtype,
           "rounds": args.rounds, "reps": args.reps, "tile": list(ops.linear_topk_tile(D, dt))}
    rec.update(measure(fns, args.rounds, args.reps))
    rec["rows_differing_from_fused32"] = float((tables[0][1] != tables[2][1]).any(1).float().mean())
    rec["rows_differing_from_composition16"] = float(
        (tables[0][1] != tables[1][1]).any(1).float().mean())
    rec["fused16_tflops"] = 2.0 * n * D * D_IN / rec["fused16_ms"] / 1e9
    for other in ("composition16", "fused32", "composition32"):
        rec["fused16_over_" + other] = rec["fused16_ms"] / rec[other + "_ms"]
    rec["fused16_within_composition16"] = bool(rec["fused16_ms"] <= rec["composition16_ms"])
    rec["fused16_peak_bytes"] = peak_above(lambda: ops.linear_topk(h16, w16, b, k))
    rec["composition16_peak_bytes"] = peak_above(
        lambda: ops.maxk_forward(F.linear(h16, w16, b16).float(), k, return_index=True))
    rec["dense_preactivation_bytes"] = 4 * n * D
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
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="f32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", *(("r22", "linear_topk_time.jsonl")
                                                    if args.dtype == "f32" else
                                                    ("r23", "linear_topk16_time.jsonl")))
    if not torch.cuda.is_available():
        sys.exit("linear_topk_time.py needs a GPU: it measures nothing without one")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.datasets.split(","):
        for k in (int(v) for v in args.ks.split(",")):
            (record if args.dtype == "f32" else record16)(name, k, args, dev)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
