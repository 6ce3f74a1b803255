"""Time of the neighbour sampler on the bench graphs: maxk_sample_neighbors, maxk_block_compact
and a full NeighborSampler.sample (its read-backs included), next to a torch restatement of the
sampler on the same device (the same keys from tensor ops, a segmented sort by three stable
sorts, the same output), and a MaxKSAGE mini-batch step (sample, forward, backward) with the
share that sampling, the per-block transpose and the aggregation take. HIP events on the launch
stream, warm-up, medians of --rounds windows of --reps calls, everything alternating inside every
round. The sampler's bytes per second are taken against 4 (S + sum n) read plus 8 sum min(n, f)
written, n the length of each seed's row. One JSON line per (dataset, fanouts, batch), appended
to --out.

  python tools/sample_time.py [--datasets reddit,ogbn-products] [--batches 1024,65536]
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
M32 = 0xFFFFFFFF


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


def fmix32(x):
    x = x & M32
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def torch_sample(ptr64, idx, seeds64, fanout, seed):
    """The sampler's three outputs from tensor ops: keys of the header's hash, a sort of every
    candidate edge by (seed position, key, edge), the first `fanout` of each segment kept."""
    lo, hi = seed & M32, (seed >> 32) & M32
    start = ptr64[seeds64]
    n = ptr64[seeds64 + 1] - start
    seg = torch.repeat_interleave(torch.arange(seeds64.numel(), device=idx.device), n)
    first = torch.cumsum(n, 0) - n
    e = start[seg] + (torch.arange(seg.numel(), device=idx.device) - first[seg])
    key = fmix32(fmix32(e ^ lo) ^ fmix32(((e * 0x9E3779B1) & M32) + hi))
    by_key = torch.argsort(key, stable=True)                 # e is ascending already
    order = by_key[torch.argsort(seg[by_key], stable=True)]  # (segment, key, edge)
    place = torch.arange(seg.numel(), device=idx.device) - first[seg]
    keep = torch.zeros(seg.numel(), dtype=torch.bool, device=idx.device)
    keep[order] = place < fanout                             # seg[order] is seg: sorted segments
    eid = e[keep]
    out_ptr = torch.zeros(seeds64.numel() + 1, dtype=torch.int64, device=idx.device)
    out_ptr[1:] = torch.cumsum(torch.clamp(n, max=fanout), 0)
    return out_ptr.to(torch.int32), idx[eid], eid.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", default="reddit,ogbn-products")
    ap.add_argument("--batches", default="1024,65536")
    ap.add_argument("--fanouts", default="10;25;15,10,5")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-reps", type=int, default=3,
                    help="calls per window of the torch restatement and the model step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "sample_time.jsonl"))
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
        for batch in [int(v) for v in args.batches.split(",")]:
            batch = min(batch, n_nodes)
            seeds = torch.randperm(n_nodes, device=dev)[:batch].to(torch.int32)
            seeds64 = seeds.long()
            lens = (ptr64[seeds64 + 1] - ptr64[seeds64])
            for fanouts in [[int(f) for f in v.split(",")] for v in args.fanouts.split(";")]:
                f = fanouts[-1]            # the layer the seeds themselves draw from
                cap = ops.sample_capacity(graph.num_edges, batch, f)
                out = (torch.empty(batch + 1, dtype=torch.int32, device=dev),
                       torch.empty(cap, dtype=torch.int32, device=dev),
                       torch.empty(cap, dtype=torch.int32, device=dev))
                scratch = torch.empty(ops.sample_scratch_bytes(batch), dtype=torch.uint8,
                                      device=dev)
                ops.sample_neighbors(graph.ptr, graph.idx, seeds, f, 1, out=out, scratch=scratch)
                m = int(out[0][-1])
                want = torch_sample(ptr64, graph.idx, seeds64, f, 1)
                assert torch.equal(want[0], out[0]) and torch.equal(want[2], out[2][:m])
                cols = out[1][:m].clone()
                cout = (torch.empty(batch + min(m, n_nodes), dtype=torch.int32, device=dev),
                        torch.empty(m, dtype=torch.int32, device=dev),
                        torch.empty(2, dtype=torch.int32, device=dev))
                cscratch = torch.empty(ops.block_compact_scratch_bytes(n_nodes),
                                       dtype=torch.uint8, device=dev)
                sampler = mk.NeighborSampler(fanouts, seed=3)
                torch.manual_seed(17)
                model = mk.MaxKSAGE(D, D, len(fanouts), 47, maxk=K, feat_drop=0.0).to(dev)
                _, _, blocks = sampler.sample(graph, seeds)
                means = [b.with_values("mean") for b in blocks]
                x_in = feats[blocks[0].src_ids.long()]
                tables = []
                for b in means:
                    sd, si = ops.maxk_forward(torch.randn(b.num_src, D, device=dev), K,
                                              return_index=True)
                    tables.append((sd.requires_grad_(True), si))
                gouts = [torch.randn(b.num_dst, D, device=dev) for b in means]

                def step():
                    _, _, bl = sampler.sample(graph, seeds)
                    model.zero_grad(set_to_none=True)
                    model(bl, feats[bl[0].src_ids.long()]).square().mean().backward()

                def transposes():
                    for b in means:
                        b._values.pop("transposed_structure", None)
                        b._values.pop("transposed_order", None)
                        b.transposed_structure()
                        b.transposed_order()

                def aggregations():
                    for b, (sd, si), g in zip(means, tables, gouts):
                        sd.grad = None
                        mk.block_spgemm(sd, si, b, D).backward(g)

                slow = args.slow_reps
                fns = {
                    "sampler_ms": (lambda: ops.sample_neighbors(
                        graph.ptr, graph.idx, seeds, f, 1, out=out, scratch=scratch), None),
                    "compact_ms": (lambda: ops.block_compact(
                        seeds, cols, n_nodes, out=cout, scratch=cscratch), None),
                    "torch_sampler_ms": (lambda: torch_sample(ptr64, graph.idx, seeds64, f, 1),
                                         slow),
                    "neighbor_sampler_ms": (lambda: sampler.sample(graph, seeds), slow),
                    "transpose_ms": (transposes, slow),
                    "aggregation_ms": (aggregations, slow),
                    "model_forward_ms": (lambda: model(blocks, x_in), slow),
                    "minibatch_step_ms": (step, slow),
                }
                aggregations()            # the cached transposes exist before they are timed
                rec = {"dataset": name, "n": n_nodes, "edges": graph.num_edges, "batch": batch,
                       "fanouts": fanouts, "sampler_fanout": f, "sampled_edges": m, "D": D,
                       "k": K, "rounds": args.rounds, "reps": args.reps, "slow_reps": slow,
                       "block_src": [b.num_src for b in blocks],
                       "block_edges": [b.num_edges for b in blocks]}
                rec.update(measure(fns, args.rounds, args.reps))
                model_bytes = 4 * (batch + int(lens.sum())) + 8 * m
                rec.update(
                    sampler_model_bytes=model_bytes,
                    sampler_gbps=model_bytes / rec["sampler_ms"] / 1e6,
                    torch_vs_sampler=rec["torch_sampler_ms"] / rec["sampler_ms"],
                    share_sampling=rec["neighbor_sampler_ms"] / rec["minibatch_step_ms"],
                    share_transpose=rec["transpose_ms"] / rec["minibatch_step_ms"],
                    share_aggregation=rec["aggregation_ms"] / rec["minibatch_step_ms"])
                emit(rec)
                del model, blocks, means, tables, gouts, fns
                torch.cuda.empty_cache()
        del graph, feats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
