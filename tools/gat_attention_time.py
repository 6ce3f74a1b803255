"""Kernel time and peak memory of the fused GAT attention (maxk_gat_attention_forward /
_backward, maxk_edge_colsum) on the bench graphs, next to the same process's composition that
MaxKGATConv runs without it (torch's two gathers, add and leaky-relu, then maxk_edge_softmax;
its backward is autograd's, index_add included) and next to maxk_edge_softmax_forward alone on
precomputed logits. HIP events on the launch stream, warm-up, the median of --rounds windows of
--reps launches, the compared calls alternating inside every round. Peak memory is
torch.cuda.max_memory_allocated over one forward and backward, above what was allocated before.

--base-lib PATH: also times maxk_edge_softmax_forward / _backward of another build of the
library (the parent commit's) in the same alternation, and compares the two builds' outputs bit
for bit: the evidence that sharing the softmax's device functions did not move the existing path.
One JSON line per dataset, appended to --out.

  python tools/gat_attention_time.py [--datasets reddit,ogbn-products] [--rounds 7] [--reps 20]
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
import torch.nn.functional as F  # noqa: E402

import maxk_kernels as mk  # noqa: E402
from maxk_kernels import _lib, graphs, ops  # noqa: E402

SLOPE = 0.2


def window(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


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


def peak(fn):
    """Peak bytes allocated while fn runs, above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def load_base(path):
    """The two softmax entry points of another build, bound like _lib binds them."""
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    for name in ("maxk_edge_softmax_forward", "maxk_edge_softmax_backward"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "gat_attention.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    base = load_base(args.base_lib) if args.base_lib else None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for name in args.datasets.split(","):
        n, _ = graphs.DATASETS[name]
        ptr, idx = graphs.bench_csr(name, device=dev)
        e = idx.numel()
        graph = mk.CSRGraph(ptr, idx)
        ptr, idx = graph.ptr, graph.idx
        rows, idx64 = graph.edge_rows(), idx.long()
        ptr_t, order = graph.transposed_structure()[0], graph.transposed_order()
        col_deg = (ptr_t[1:] - ptr_t[:-1])
        el = graphs.features(n, 1, seed=97, device=dev).reshape(n)
        er = graphs.features(n, 1, seed=98, device=dev).reshape(n)
        g = graphs.features(e, 1, seed=99, device=dev).reshape(e)
        alpha, ge = torch.empty(e, device=dev), torch.empty(e, device=dev)
        ger, gel = torch.empty(n, device=dev), torch.empty(n, device=dev)
        x = F.leaky_relu(el[idx64] + er[rows], SLOPE)        # the materialised logits
        y, gx = torch.empty(e, device=dev), torch.empty(e, device=dev)
        ops.edge_softmax(ptr, x, out=y)
        ops.gat_attention(ptr, idx, el, er, SLOPE, out=alpha)
        same = bool(torch.equal(alpha.view(torch.int32), y.view(torch.int32)))
        elt, ert = el.clone().requires_grad_(True), er.clone().requires_grad_(True)
        state = {}

        def comp_fwd():
            sc = F.leaky_relu(elt[idx64] + ert[rows], SLOPE)
            state["alpha"] = mk.edge_softmax(graph, sc)

        def comp_bwd():
            elt.grad = ert.grad = None
            state["alpha"].backward(g, retain_graph=True)

        def fused_step():
            elt.grad = ert.grad = None
            mk.gat_attention(graph, elt, ert, SLOPE).backward(g)

        def comp_step():
            comp_fwd()
            comp_bwd()
            state.clear()

        comp_fwd()
        fns = {
            "fused_fwd_ms": lambda: ops.gat_attention(ptr, idx, el, er, SLOPE, out=alpha),
            "softmax_fwd_ms": lambda: ops.edge_softmax(ptr, x, out=y),
            "comp_fwd_ms": comp_fwd,
            "fused_bwd_ms": lambda: ops.gat_attention_backward(ptr, idx, el, er, SLOPE, alpha, g,
                                                               out=(ge, ger)),
            "colsum_ms": lambda: ops.edge_colsum(ptr_t, order, ge, out=gel),
            "softmax_bwd_ms": lambda: ops.edge_softmax_backward(ptr, y, g, out=gx),
            "comp_bwd_ms": comp_bwd,
        }
        if base is not None:
            yb, gxb = torch.empty(e, device=dev), torch.empty(e, device=dev)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
            fns["base_softmax_fwd_ms"] = lambda: base.maxk_edge_softmax_forward(
                p(ptr), p(x), p(yb), n, e, st)
            fns["base_softmax_bwd_ms"] = lambda: base.maxk_edge_softmax_backward(
                p(ptr), p(y), p(g), p(gxb), n, e, st)
        rec = {"dataset": name, "n": n, "edges": e, "edges_per_row": e / n,
               "longest_row": int(graph.in_degrees().max()), "longest_column": int(col_deg.max()),
               "negative_slope": SLOPE, "rounds": args.rounds, "reps": args.reps,
               "fused_alpha_bit_equal_to_softmax_of_logits": same}
        rec.update(measure(fns, args.rounds, args.reps))
        state.clear()
        if base is not None:
            torch.cuda.synchronize()
            rec["base_lib"] = os.path.basename(args.base_lib)
            rec["base_lib_sha256"] = _lib.lib_sha256(args.base_lib)
            rec["lib_sha256"] = _lib.lib_sha256()
            rec["softmax_fwd_bit_equal_to_base"] = bool(torch.equal(y.view(torch.int32),
                                                                    yb.view(torch.int32)))
            rec["softmax_bwd_bit_equal_to_base"] = bool(torch.equal(gx.view(torch.int32),
                                                                    gxb.view(torch.int32)))
            rec["softmax_fwd_vs_base"] = rec["softmax_fwd_ms"] / rec["base_softmax_fwd_ms"]
            rec["softmax_bwd_vs_base"] = rec["softmax_bwd_ms"] / rec["base_softmax_bwd_ms"]
        rec["fused_bwd_total_ms"] = rec["fused_bwd_ms"] + rec["colsum_ms"]
        rec.update(
            fused_fwd_vs_softmax_alone=rec["fused_fwd_ms"] / rec["softmax_fwd_ms"],
            fwd_speedup_vs_composition=rec["comp_fwd_ms"] / rec["fused_fwd_ms"],
            bwd_speedup_vs_composition=rec["comp_bwd_ms"] / rec["fused_bwd_total_ms"],
            fwd_model_bytes=8 * e + 12 * n, fused_fwd_tb_per_s=(8 * e + 12 * n) /
            rec["fused_fwd_ms"] * 1e-9,
            fused_bwd_tb_per_s=(16 * e + 16 * n) / rec["fused_bwd_ms"] * 1e-9,
            colsum_tb_per_s=(8 * e + 8 * n) / rec["colsum_ms"] * 1e-9)
        del x, y, gx, alpha, ge
        rec["fused_peak_bytes"] = peak(fused_step)
        rec["comp_peak_bytes"] = peak(comp_step)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del graph, rows, idx64, g, elt, ert, ptr_t, order
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
