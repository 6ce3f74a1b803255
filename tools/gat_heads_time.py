"""Kernel time and peak memory of multi-head GAT on the bench graphs: the multi-head aggregation
(maxk_heads_aggregate_forward / _backward), the head-batched attention, and the whole layer step
(attention plus aggregation, forward plus backward through autograd), next to the same process's
composition that was the only way to H heads before: per head one single-head attention and one
spgemm(sp_data * head_mask, sp_index, graph, D, edge_weight=alpha[h]), with autograd's backward.
The composition is timed twice, before and after the new path; its own spread is the margin.
Reported without a bar: the single-head plan kernels at the same k (SpGEMM forward, SSpMM plus
SDDMM), which say what a planned multi-head kernel could still win, and the peak memory of both
steps. HIP events on the launch stream, warm-up, medians of --rounds windows of --reps calls
(--comp-reps for the composition step), everything alternating inside every round.

--base-lib PATH: also times the two softmax kernels and the three single-head GAT kernels of
another build of the library (the parent commit's) in the same alternation and compares the
outputs bit for bit: the evidence that the head coordinate did not move the single-head path.
One JSON line per dataset and (H, k), appended to --out.

  python tools/gat_heads_time.py [--datasets reddit,ogbn-products] [--shapes 4x16,8x16,8x32]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spgemm-gnn_amd"))
import torch  # noqa: E402

import maxk_kernels as mk  # noqa: E402
from maxk_kernels import _lib, graphs, ops  # noqa: E402

SLOPE = 0.2
D = 256
BASE_SYMBOLS = ("maxk_edge_softmax_forward", "maxk_edge_softmax_backward",
                "maxk_gat_attention_forward", "maxk_gat_attention_backward", "maxk_edge_colsum")


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


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def load_base(path):
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for name in BASE_SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def existing_paths(base, graph, rounds, reps, dev):
    """The five existing kernels of this build and of `base`, alternating; outputs bit for bit."""
    ptr, idx, n, e = graph.ptr, graph.idx, graph.num_nodes, graph.num_edges
    ptr_t, order = graph.transposed_structure()[0], graph.transposed_order()
    el = graphs.features(n, 1, seed=97, device=dev).reshape(n)
    er = graphs.features(n, 1, seed=98, device=dev).reshape(n)
    g = torch.randn(e, device=dev, generator=torch.Generator(dev).manual_seed(99))
    x = torch.nn.functional.leaky_relu(el[idx.long()] + er[graph.edge_rows()], SLOPE)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    out = {tag: {k: torch.empty(e if k in ("y", "gx", "alpha", "ge") else n, device=dev)
                 for k in ("y", "gx", "alpha", "ge", "ger", "gel")} for tag in ("cand", "base")}
    fns = {}
    for tag, lib in (("cand", _lib.lib), ("base", base)):
        o = out[tag]
        calls = {
            "softmax_fwd": lambda lib=lib, o=o: lib.maxk_edge_softmax_forward(
                p(ptr), p(x), p(o["y"]), n, e, st),
            "softmax_bwd": lambda lib=lib, o=o: lib.maxk_edge_softmax_backward(
                p(ptr), p(o["y"]), p(g), p(o["gx"]), n, e, st),
            "gat_fwd": lambda lib=lib, o=o: lib.maxk_gat_attention_forward(
                p(ptr), p(idx), p(el), p(er), SLOPE, p(o["alpha"]), n, n, e, st),
            "gat_bwd": lambda lib=lib, o=o: lib.maxk_gat_attention_backward(
                p(ptr), p(idx), p(el), p(er), SLOPE, p(o["alpha"]), p(g), p(o["ge"]),
                p(o["ger"]), n, n, e, st),
            "colsum": lambda lib=lib, o=o: lib.maxk_edge_colsum(
                p(ptr_t), p(order), p(o["ge"]), p(o["gel"]), n, e, st),
        }
        for key, fn in calls.items():
            fns[f"{tag}_{key}_ms"] = (fn, None)
    rec = measure(fns, rounds, reps)
    torch.cuda.synchronize()
    rec["existing_outputs_bit_equal_to_base"] = all(
        same_bits(out["cand"][k], out["base"][k]) for k in out["cand"])
    for key in ("softmax_fwd", "softmax_bwd", "gat_fwd", "gat_bwd", "colsum"):
        rec[f"{key}_vs_base"] = rec[f"cand_{key}_ms"] / rec[f"base_{key}_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--shapes", default="4x16,8x16,8x32", help="HxK pairs at D = 256")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--comp-reps", type=int, default=5)
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "gat_heads.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    base = load_base(args.base_lib) if args.base_lib else None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.datasets.split(","):
        n, _ = graphs.DATASETS[name]
        ptr, idx = graphs.bench_csr(name, device=dev)
        graph = mk.CSRGraph(ptr, idx).with_values("sum")
        e = graph.num_edges
        ptr_t, idx_t, _ = graph.transposed_structure()
        order = graph.transposed_order()
        gout = graphs.features(n, D, seed=96, device=dev)
        x = graphs.features(n, D, seed=95, device=dev)
        existing = {}
        if base is not None:
            existing = existing_paths(base, graph, args.rounds, args.reps, dev)
            existing.update(base_lib=os.path.basename(args.base_lib),
                            base_lib_sha256=_lib.lib_sha256(args.base_lib),
                            lib_sha256=_lib.lib_sha256())
        for shape in args.shapes.split(","):
            H, k = (int(v) for v in shape.split("x"))
            Fh = D // H
            sp_data, sp_index = ops.maxk_forward(x, k, return_index=True)
            masks = [(sp_index // Fh == h).to(torch.float32) for h in range(H)]
            el = graphs.features(n, H, seed=97, device=dev).t().contiguous().requires_grad_(True)
            er = graphs.features(n, H, seed=98, device=dev).t().contiguous().requires_grad_(True)
            sp = sp_data.clone().requires_grad_(True)
            alpha = ops.gat_attention_heads(graph.ptr, graph.idx, el.detach(), er.detach(), SLOPE)
            galpha = torch.randn((H, e), device=dev,
                                 generator=torch.Generator(dev).manual_seed(99))
            out = torch.empty((n, D), device=dev)
            ge, ger = torch.empty((H, e), device=dev), torch.empty((H, n), device=dev)
            gel = torch.empty((H, n), device=dev)
            plan = graph.plan(D, k)

            def new_step():
                el.grad = er.grad = sp.grad = None
                a = mk.gat_attention_heads(graph, el, er, SLOPE)
                mk.heads_aggregate(graph, a, sp, sp_index, D).backward(gout)

            def comp_step():
                el.grad = er.grad = sp.grad = None
                y = None
                for h in range(H):
                    a = mk.gat_attention(graph, el[h], er[h], SLOPE)
                    t = mk.spgemm(sp * masks[h], sp_index, graph, D, edge_weight=a)
                    y = t if y is None else y + t
                y.backward(gout)

            fns = {
                "comp_step_before_ms": (comp_step, args.comp_reps),
                "heads_fwd_ms": (lambda: ops.heads_aggregate(graph.ptr, graph.idx, alpha, sp_data,
                                                             sp_index, D, out=out), None),
                "heads_bwd_ms": (lambda: ops.heads_aggregate_backward(
                    ptr_t, idx_t, order, alpha, gout, sp_data, sp_index), None),
                "attn_fwd_ms": (lambda: ops.gat_attention_heads(
                    graph.ptr, graph.idx, el.detach(), er.detach(), SLOPE, out=alpha), None),
                "attn_bwd_ms": (lambda: ops.gat_attention_backward_heads(
                    graph.ptr, graph.idx, el.detach(), er.detach(), SLOPE, alpha, galpha,
                    out=(ge, ger)), None),
                "attn_colsum_ms": (lambda: ops.edge_colsum_heads(ptr_t, order, ge, out=gel), None),
                "new_step_ms": (new_step, None),
                "plan_spgemm_fwd_ms": (lambda: plan.forward(sp_data, sp_index), None),
                "plan_sspmm_bwd_ms": (lambda: plan.backward(gout, sp_index), None),
                "sddmm_ms": (lambda: ops.spgemm_edge_grad(graph.ptr, graph.idx, gout, sp_data,
                                                          sp_index, n, e, k, D), None),
                "comp_step_after_ms": (comp_step, args.comp_reps),
            }
            rec = {"dataset": name, "n": n, "edges": e, "D": D, "num_heads": H, "k": k,
                   "rounds": args.rounds, "reps": args.reps, "comp_reps": args.comp_reps}
            rec.update(measure(fns, args.rounds, args.reps))
            comp = min(rec["comp_step_before_ms"], rec["comp_step_after_ms"])
            rec.update(
                step_speedup_vs_faster_composition=comp / rec["new_step_ms"],
                heads_fwd_vs_plan_fwd=rec["heads_fwd_ms"] / rec["plan_spgemm_fwd_ms"],
                heads_bwd_vs_plan_bwd_plus_sddmm=rec["heads_bwd_ms"] /
                (rec["plan_sspmm_bwd_ms"] + rec["sddmm_ms"]))
            rec["new_step_peak_bytes"] = peak(new_step)
            rec["comp_step_peak_bytes"] = peak(comp_step)
            rec.update(existing)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            masks = alpha = galpha = out = ge = ger = gel = plan = None
            torch.cuda.empty_cache()
        del graph, gout, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
