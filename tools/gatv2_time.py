"""Kernel time and peak memory of the MaxK GATv2 attention on the bench graphs at D = 256: the four
kernels (score forward, softmax over the heads forward + backward, score backward over the rows and
over the columns), the attention step forward plus backward through autograd, and next to them in
the same process
  * maxk_sddmm_edge_grad at the same k, which makes the same gathers per edge (the expectation to
    confirm or refute: the score forward costs the order of it);
  * a torch composition of the same MaxK score ([E, k] gathers, scatter_add per head, autograd's
    backward with index_add), forward plus backward, against score forward + both score backwards;
  * on --dense-dataset (the largest bench shape whose [E, D] messages fit): GATv2's dense [E, D]
    score in torch, forward plus backward, against the new path's score kernels on that graph.
HIP events on the launch stream, warm-up, medians of --rounds windows of --reps calls (--comp-reps
for the torch steps), everything alternating inside every round. A torch step that does not fit,
or that torch refuses at that size, is recorded as null with its error. One JSON line per dataset
and (H, k), appended to --out.

  python tools/gatv2_time.py [--datasets reddit,ogbn-products] [--shapes 4x16,8x32]
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

import maxk_kernels as mk  # noqa: E402
from maxk_kernels import graphs, ops  # noqa: E402

SLOPE = 0.2
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
    """fns: key -> (fn, reps or None). Medians and [min, max] of `rounds` windows per key; a
    function that raises in its warm-up (out of memory, a size limit of torch) is dropped and
    recorded as null with the error."""
    rec, live = {}, {}
    for key, (fn, r) in fns.items():
        try:
            fn()
            fn()
            live[key] = (fn, r)
        except RuntimeError as exc:   # out of memory, or a torch kernel's own size limit
            rec[key], rec[key.replace("_ms", "_error")] = None, str(exc).split(".")[0][:120]
            torch.cuda.empty_cache()
    torch.cuda.synchronize()
    times = {key: [] for key in live}
    for _ in range(rounds):
        for key, (fn, r) in live.items():
            times[key].append(window(fn, r or reps))
    for key, ts in times.items():
        rec[key] = statistics.median(ts)
        rec[key.replace("_ms", "_min_max_ms")] = [min(ts), max(ts)]
    return rec


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        fn()
    except RuntimeError:
        torch.cuda.empty_cache()
        return None
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def setup(name, H, k, dev):
    n, _ = graphs.DATASETS[name]
    ptr, idx = graphs.bench_csr(name, device=dev)
    graph = mk.CSRGraph(ptr, idx)
    fs = graphs.features(n, D, seed=95, device=dev)
    fd = graphs.features(n, D, seed=94, device=dev).requires_grad_(True)
    attn = (graphs.features(H, D // H, seed=93, device=dev) * 0.3).requires_grad_(True)
    sp_data, sp_index = ops.maxk_forward(fs, k, return_index=True)
    sp = sp_data.clone().requires_grad_(True)
    g = torch.randn((H, graph.num_edges), device=dev,
                    generator=torch.Generator(dev).manual_seed(99))
    return n, graph, fs, fd, attn, sp, sp_index, g


def score_fns(graph, fd, attn, sp, sp_index, g, n, k, reps_torch, dense_fs=None):
    """The timed functions of one (graph, H, k): kernels, steps and the torch compositions."""
    H, e = g.shape
    dev = g.device
    ptr, idx = graph.ptr, graph.idx
    ptr_t, idx_t, _ = graph.transposed_structure()
    order = graph.transposed_order()
    spd, fdd, attnd = sp.detach(), fd.detach(), attn.detach()
    logits, alpha, gl = (torch.empty((H, e), device=dev) for _ in range(3))
    gfd, gattn, gsp = torch.empty_like(fdd), torch.empty_like(attnd), torch.empty_like(spd)
    scratch = torch.empty(ops.gatv2_scratch_bytes(n, D), dtype=torch.uint8, device=dev)
    gout = graphs.features(n, D, seed=96, device=dev)
    rows, cols = graph.edge_rows(), idx.long()

    def score_fwd():
        ops.gatv2_score(ptr, idx, spd, sp_index, fdd, attnd, SLOPE, out=logits)

    def bwd_rows():
        ops.gatv2_score_backward_rows(ptr, idx, spd, sp_index, fdd, attnd, SLOPE, g,
                                      out=(gfd, gattn), scratch=scratch)

    def bwd_cols():
        ops.gatv2_score_backward_cols(ptr_t, idx_t, order, spd, sp_index, fdd, attnd, SLOPE, g,
                                      out=gsp)

    def score_kernels():
        score_fwd()
        bwd_rows()
        bwd_cols()

    def attention_step():
        sp.grad = fd.grad = attn.grad = None
        mk.gatv2_attention(graph, sp, sp_index, fd, attn, SLOPE).backward(g)

    def torch_maxk_score():
        sp.grad = fd.grad = attn.grad = None
        s = sp_index[cols].long()                                   # [E, k]
        f = fd[rows[:, None], s]
        t = attn.reshape(-1)[s] * (F.leaky_relu(sp[cols] + f, SLOPE) - F.leaky_relu(f, SLOPE))
        delta = torch.zeros((e, H), device=dev).scatter_add_(1, s // (D // H), t)
        delta.backward(g.t())

    fns = {
        "score_fwd_ms": (score_fwd, None),
        "softmax_fwd_ms": (lambda: ops.edge_softmax_heads(ptr, logits, out=alpha), None),
        "softmax_bwd_ms": (lambda: ops.edge_softmax_backward_heads(ptr, alpha, g, out=gl), None),
        "score_bwd_rows_ms": (bwd_rows, None),
        "score_bwd_cols_ms": (bwd_cols, None),
        "sddmm_ms": (lambda: ops.spgemm_edge_grad(ptr, idx, gout, spd, sp_index, n, e, k, D), None),
        "score_kernels_ms": (score_kernels, None),
        "attention_step_ms": (attention_step, None),
        "torch_maxk_score_step_ms": (torch_maxk_score, reps_torch),
    }
    peaks = {"attention_step": attention_step, "score_kernels": score_kernels,
             "torch_maxk_score_step": torch_maxk_score}
    if dense_fs is not None:
        xs = dense_fs.clone().requires_grad_(True)

        def torch_dense_score():
            xs.grad = fd.grad = attn.grad = None
            z = F.leaky_relu(xs[cols] + fd[rows], SLOPE)             # [E, D]
            (z * attn.reshape(-1)).view(e, H, D // H).sum(-1).backward(g.t())

        fns["torch_dense_score_step_ms"] = (torch_dense_score, reps_torch)
        peaks["torch_dense_score_step"] = torch_dense_score
    return fns, peaks


def record(name, H, k, args, dev, dense):
    n, graph, fs, fd, attn, sp, sp_index, g = setup(name, H, k, dev)
    fns, peaks = score_fns(graph, fd, attn, sp, sp_index, g, n, k, args.comp_reps,
                           dense_fs=fs if dense else None)
    rec = {"dataset": name, "n": n, "edges": graph.num_edges, "D": D, "num_heads": H, "k": k,
           "rounds": args.rounds, "reps": args.reps, "comp_reps": args.comp_reps}
    rec.update(measure(fns, args.rounds, args.reps))
    rec["score_fwd_vs_sddmm"] = rec["score_fwd_ms"] / rec["sddmm_ms"]
    for key in ("torch_maxk_score_step_ms", "torch_dense_score_step_ms"):
        if rec.get(key):
            rec[key.replace("_step_ms", "_vs_score_kernels")] = rec[key] / rec["score_kernels_ms"]
    for key, fn in peaks.items():
        rec[key + "_peak_bytes"] = peak(fn)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--dense-dataset", default="yelp")
    ap.add_argument("--shapes", default="4x16,8x32", help="HxK pairs at D = 256")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--comp-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "gatv2_time.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gatv2_time.py needs a GPU: it measures nothing without one")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    for name in args.datasets.split(","):
        for H, k in shapes:
            record(name, H, k, args, dev, dense=False)
            torch.cuda.empty_cache()
    if args.dense_dataset:
        for H, k in shapes:
            record(args.dense_dataset, H, k, args, dev, dense=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
