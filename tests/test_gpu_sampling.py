"""GPU: maxk_sample_neighbors and maxk_block_compact against the numpy restatements of
tests/sampling.py, bit for bit (the selection rule is part of the ABI); their output contract on
guarded, poisoned buffers; capture; the block aggregation and its autograd against float64; and
MaxKSAGEConv / MaxKSAGE on blocks. Two graphs serve the module: the 600-row graph of the
multi-head tests (hub row 5,000, hub column 3,000) and a 300 x 900 rectangular one whose rows sit
at f - 1, f, f + 1 of every fanout and on both sides of every limit
(tests/test_sampling_capi.py checks those preconditions). Both scans run at the lengths of
tests/scan.py. The last test closes over the compiled maxk_sp:: instantiations and the maxk_scan::
kernels the two entry points launch.

Worst error / bound figures print with -s."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gat_heads as gh
import maxk_kernels as mk
import sampling as sp
import scan
from arena import POISONS, arena
from maxk_kernels import _lib, ops

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_instantiations_sample.txt")
COVERED = set()      # kernel names launched by a case that went on to pass
P = ctypes.c_void_p
lib = _lib.lib
U = 2.0 ** -24


def dev_of(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)      # a copy: the cached arrays are read-only


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape,
                                                                 got.dtype, want.dtype)
    diff = got != want
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def compiled():
    """The maxk_sp:: fixture and the maxk_scan:: kernels the two entry points launch."""
    with open(FIXTURE) as f:
        return {ln.strip() for ln in f if ln.strip()} | set(sp.SCAN_KERNELS)


def sampler_names(fanout):
    names = set(sp.SAMPLER_KERNELS) | {sp.sample_kernel_name(fanout)}
    assert names <= compiled(), names
    return names


@functools.lru_cache(maxsize=None)
def graph_dev(name, dev):
    ptr, idx, num_cols = sp.GRAPHS[name]()
    return dev_of(ptr, dev), dev_of(idx, dev), num_cols


def csr_graph(name, dev, val=None):
    ptr, idx, num_cols = graph_dev(name, dev)
    if num_cols != ptr.numel() - 1:      # a rectangular parent is a Block: it knows its columns
        return mk.Block(ptr, idx, val, num_src=num_cols)
    return mk.CSRGraph(ptr, idx, val)


def run_sampler(name, dev, seeds, fanout, seed):
    """The three outputs as numpy arrays, out_col / out_eid cut to out_ptr[S]."""
    ptr, idx, _ = graph_dev(name, dev)
    out_ptr, col, eid = ops.sample_neighbors(ptr, idx, dev_of(seeds, dev), fanout, seed)
    out_ptr = out_ptr.cpu().numpy()
    m = int(out_ptr[-1])
    assert m <= col.numel()
    return out_ptr, col.cpu().numpy()[:m], eid.cpu().numpy()[:m]


def test_limits_are_the_restated_ones(gpu):
    assert ops.sample_row_limits() == sp.LIMITS


# ------------------------------------------------------------------ 1. sampler, bit for bit
SAMPLER_CASES = [(name, i) for name in sorted(sp.GRAPHS) for i in range(len(sp.FANOUTS) + 2)]


@pytest.mark.parametrize("name,which", SAMPLER_CASES)
def test_sampler_matches_the_restatement_bit_for_bit(gpu, name, which):
    ptr, idx, _ = sp.GRAPHS[name]()
    fanout = sp.fanouts_for(ptr)[which]
    names = sampler_names(fanout)
    for set_name, seeds in sp.seed_sets(ptr).items():
        got = run_sampler(name, gpu, seeds, fanout, seed=0x5EED0000 + which)
        want = sp.sample_ref(ptr, idx, seeds, fanout, 0x5EED0000 + which)
        for g, w, what in zip(got, want, ("out_ptr", "out_col", "out_eid")):
            same(g, w, f"{name} fanout {fanout} seeds {set_name}: {what}")
    COVERED.update(names)


def test_tie_break_seed_is_decided_by_the_edge_number(gpu):
    seed, fanout, e0, e1 = sp.tie_break_case()
    ptr, idx, _ = sp.square_graph()
    for seeds in (sp.seed_sets(ptr)["hub"], sp.seed_sets(ptr)["all"]):
        got = run_sampler("square", gpu, seeds, fanout, seed)
        want = sp.sample_ref(ptr, idx, seeds, fanout, seed)
        for g, w, what in zip(got, want, ("out_ptr", "out_col", "out_eid")):
            same(g, w, f"tie-break seed: {what}")
        assert e0 in got[2] and e1 not in got[2]
    COVERED.update(sampler_names(fanout))


def test_a_rows_sample_does_not_depend_on_the_batch(gpu):
    for name in sorted(sp.GRAPHS):
        ptr, _, _ = sp.GRAPHS[name]()
        sets = sp.seed_sets(ptr)
        for fanout in (2, 25):
            a_ptr, _, a_eid = run_sampler(name, gpu, sets["all"], fanout, 99)
            p_ptr, _, p_eid = run_sampler(name, gpu, sets["permutation"], fanout, 99)
            where = np.argsort(sets["permutation"])
            for r in (0, 5, 17, sp.hub_row(ptr), sp.empty_row(ptr), ptr.size - 2):
                alone = run_sampler(name, gpu, np.array([r], np.int32), fanout, 99)[2]
                same(a_eid[a_ptr[r]:a_ptr[r + 1]], alone, f"{name} row {r}: all rows vs alone")
                i = where[r]
                same(p_eid[p_ptr[i]:p_ptr[i + 1]], alone, f"{name} row {r}: permuted vs alone")


def test_the_high_word_of_the_seed_matters(gpu):
    ptr, _, _ = sp.square_graph()
    seeds = sp.seed_sets(ptr)["all"]
    a = run_sampler("square", gpu, seeds, 10, 0x1234)
    b = run_sampler("square", gpu, seeds, 10, 0x1234 + (1 << 32))
    same(a[0], b[0], "out_ptr")
    assert not np.array_equal(a[2], b[2])
    # a seed is taken modulo 2^64
    same(run_sampler("square", gpu, seeds, 10, -1)[2],
         run_sampler("square", gpu, seeds, 10, 2 ** 64 - 1)[2], "seed modulo 2^64")


# ------------------------------------------------------------------ 2. compaction
@pytest.mark.parametrize("name", sorted(sp.GRAPHS))
def test_compaction_matches_the_restatement_bit_for_bit(gpu, name):
    ptr, idx, num_cols = sp.GRAPHS[name]()
    sets = sp.seed_sets(ptr)
    cases = [(sets["all"], -1), (sets["all"], 10), (sets["permutation"][:77], 25),
             (sets["permutation"][:77], 2), (sets["hub"], 64), (sets["empty_row"], 10),
             (sets["none"], 10)]
    for seeds, fanout in cases:
        _, col, _ = sp.sample_ref(ptr, idx, seeds, fanout, 7)
        src, local, counts = ops.block_compact(dev_of(seeds, gpu), dev_of(col, gpu), num_cols)
        w_src, w_local, w_counts = sp.compact_ref(seeds, col, num_cols)
        what = f"{name} {len(seeds)} seeds fanout {fanout}"
        assert tuple(counts.tolist()) == w_counts, what
        same(src.cpu().numpy()[:w_counts[0]], w_src, what + ": src_ids")
        same(local.cpu().numpy(), w_local, what + ": local_col")
        s2, l2 = mk.block_compact(dev_of(seeds, gpu), dev_of(col, gpu), num_cols)
        same(s2.cpu().numpy()[l2.cpu().numpy()], col, what + ": src_ids[local_col] == out_col")
    COVERED.update(sp.COMPACT_KERNELS)


def test_duplicate_seeds_raise(gpu):
    ptr, idx, num_cols = sp.square_graph()
    seeds = np.array([30, 40, 30, 50], np.int32)
    _, col, _ = sp.sample_ref(ptr, idx, seeds, 5, 1)
    src, local, counts = ops.block_compact(dev_of(seeds, gpu), dev_of(col, gpu), num_cols)
    w_src, w_local, w_counts = sp.compact_ref(seeds, col, num_cols)
    assert tuple(counts.tolist()) == w_counts and w_counts[1] == 3
    same(src.cpu().numpy()[:w_counts[0]], w_src, "src_ids with a repeated seed")
    same(local.cpu().numpy(), w_local, "local_col with a repeated seed")
    with pytest.raises(ValueError, match="seeds must be distinct"):
        mk.block_compact(dev_of(seeds, gpu), dev_of(col, gpu), num_cols)
    with pytest.raises(ValueError, match="seeds must be distinct"):
        mk.to_block(csr_graph("square", gpu), dev_of(seeds, gpu), 5, 1)


# ------------------------------------------------------------------ 3. output contract
@pytest.mark.parametrize("poison", POISONS)
def test_output_contract(gpu, poison):
    """Poisoned outputs are fully written in their valid ranges, nothing is written past
    out_ptr[S], the bound or the reported scratch size, and scratch that arrives dirty (both
    poisons) changes no output."""
    for name, fanout in (("square", 10), ("rect", 25), ("square", -1)):
        ptr, idx, num_cols = sp.GRAPHS[name]()
        ptr_d, idx_d, _ = graph_dev(name, gpu)
        seeds = sp.seed_sets(ptr)["permutation"][:123]
        s, e = len(seeds), idx.size
        cap = ops.sample_capacity(e, s, fanout)
        w_ptr, w_col, w_eid = sp.sample_ref(ptr, idx, seeds, fanout, 21)
        m = int(w_ptr[-1])
        assert m < cap                            # there is a range that must stay untouched
        a_ptr = arena((1, s + 1, torch.int32), gpu, poison)
        a_col, a_eid = (arena((1, cap, torch.int32), gpu, poison) for _ in range(2))
        sb = ops.sample_scratch_bytes(s)
        a_scr = arena(sb, gpu, poison)
        seeds_d = dev_of(seeds, gpu)
        assert lib.maxk_sample_neighbors(P(ptr_d.data_ptr()), P(idx_d.data_ptr()),
                                         P(seeds_d.data_ptr()), P(a_ptr.ptr), P(a_col.ptr),
                                         P(a_eid.ptr), cap, P(a_scr.ptr), sb, ptr.size - 1, e, s,
                                         fanout, 21, None) == 0
        torch.cuda.synchronize()
        for a, what in ((a_ptr, "out_ptr"), (a_col, "out_col"), (a_eid, "out_eid"),
                        (a_scr, "scratch")):
            assert a.check() is None, (name, fanout, what, a.check())
        same(a_ptr.payload.cpu().numpy()[0], w_ptr, "out_ptr in the arena")
        poison32 = np.frombuffer(bytes([poison] * 4), np.int32)[0]
        for a, want, what in ((a_col, w_col, "out_col"), (a_eid, w_eid, "out_eid")):
            got = a.payload.cpu().numpy()[0]
            same(got[:m], want, what + " in the arena")
            assert (got[m:] == poison32).all(), what + " written past out_ptr[S]"

        # compaction on the sampler's output
        cap_src = s + min(m, num_cols)
        w_src, w_local, w_counts = sp.compact_ref(seeds, w_col, num_cols)
        assert w_counts[0] < cap_src
        a_src = arena((1, cap_src, torch.int32), gpu, poison)
        a_loc = arena((1, m, torch.int32), gpu, poison)
        a_cnt = arena((1, 2, torch.int32), gpu, poison)
        cb = ops.block_compact_scratch_bytes(num_cols)
        a_cs = arena(cb, gpu, poison)
        col_d = dev_of(w_col, gpu)
        assert lib.maxk_block_compact(P(seeds_d.data_ptr()), P(col_d.data_ptr()), P(a_src.ptr),
                                      cap_src, P(a_loc.ptr), P(a_cnt.ptr), P(a_cs.ptr), cb, s, m,
                                      num_cols, None) == 0
        torch.cuda.synchronize()
        for a, what in ((a_src, "src_ids"), (a_loc, "local_col"), (a_cnt, "counts"),
                        (a_cs, "scratch")):
            assert a.check() is None, (name, fanout, what, a.check())
        got = a_src.payload.cpu().numpy()[0]
        same(got[:w_counts[0]], w_src, "src_ids in the arena")
        assert (got[w_counts[0]:] == poison32).all(), "src_ids written past num_src"
        same(a_loc.payload.cpu().numpy()[0], w_local, "local_col in the arena")
        assert tuple(a_cnt.payload.cpu().numpy()[0].tolist()) == w_counts
        COVERED.update(sampler_names(fanout))
    COVERED.update(sp.COMPACT_KERNELS)


def test_no_seeds_and_a_bound_that_is_too_small(gpu):
    ptr_d, idx_d, _ = graph_dev("square", gpu)
    ptr, idx, _ = sp.square_graph()
    out_ptr, col, eid = ops.sample_neighbors(ptr_d, idx_d, dev_of(sp.seed_sets(ptr)["none"], gpu),
                                             10, 1)
    assert out_ptr.tolist() == [0] and col.numel() == 0 == eid.numel()
    # repeated seeds can exceed the bound for distinct ones: nothing is written past it, and
    # out_ptr tells
    hub = sp.hub_row(ptr)
    reps = idx.size // 5000 + 1               # more edges than the graph has
    seeds = np.full(reps, hub, np.int32)
    a_col, a_eid = (arena((1, 5000, torch.int32), gpu, 0xFF) for _ in range(2))
    out = (torch.empty(reps + 1, dtype=torch.int32, device=gpu), a_col.payload[0],
           a_eid.payload[0])
    ops.sample_neighbors(ptr_d, idx_d, dev_of(seeds, gpu), -1, 1, out=out)
    torch.cuda.synchronize()
    assert out[0].tolist() == [5000 * i for i in range(reps + 1)]
    assert a_col.check() is None and a_eid.check() is None
    same(a_eid.payload.cpu().numpy()[0], np.arange(ptr[hub], ptr[hub + 1], dtype=np.int32),
         "the first seed's edges")
    with pytest.raises(ValueError, match="seeds repeat"):
        mk.sample_neighbors(csr_graph("square", gpu), dev_of(seeds, gpu), -1, 1)


# ------------------------------------------------------------------ 4. capture
def test_both_calls_replay_from_one_captured_graph(gpu):
    ptr, idx, num_cols = sp.square_graph()
    ptr_d, idx_d, _ = graph_dev("square", gpu)
    rows = sp.seed_sets(ptr)["permutation"][:200]
    sets = [rows, rows[::-1].copy(), np.roll(rows, 7)]      # one row set: one edge count
    fanout, seed = 10, 5
    refs = []
    for s in sets:
        w = sp.sample_ref(ptr, idx, s, fanout, seed)
        refs.append(w + sp.compact_ref(s, w[1], num_cols))
    m = int(refs[0][0][-1])
    assert all(int(r[0][-1]) == m for r in refs) and not np.array_equal(refs[0][2], refs[1][2])
    s = len(rows)
    cap = ops.sample_capacity(idx.size, s, fanout)
    seeds_d = dev_of(sets[0], gpu)
    out = (torch.empty(s + 1, dtype=torch.int32, device=gpu),
           torch.empty(cap, dtype=torch.int32, device=gpu),
           torch.empty(cap, dtype=torch.int32, device=gpu))
    scratch = torch.empty(ops.sample_scratch_bytes(s), dtype=torch.uint8, device=gpu)
    cout = (torch.empty(s + min(m, num_cols), dtype=torch.int32, device=gpu),
            torch.empty(m, dtype=torch.int32, device=gpu),
            torch.empty(2, dtype=torch.int32, device=gpu))
    cscratch = torch.empty(ops.block_compact_scratch_bytes(num_cols), dtype=torch.uint8,
                           device=gpu)

    def step():
        ops.sample_neighbors(ptr_d, idx_d, seeds_d, fanout, seed, out=out, scratch=scratch)
        ops.block_compact(seeds_d, out[1][:m], num_cols, out=cout, scratch=cscratch)

    step()                                     # eager once: equal to the restatement
    torch.cuda.synchronize()
    same(out[2].cpu().numpy()[:m], refs[0][2], "eager out_eid")
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        step()
    for which in (1, 2, 0, 1):
        seeds_d.copy_(dev_of(sets[which], gpu))
        for t in out + cout:
            t.fill_(-7)
        scratch.fill_(0x5A), cscratch.fill_(0xFF)
        cg.replay()
        torch.cuda.synchronize()
        w_ptr, w_col, w_eid, w_src, w_local, w_counts = refs[which]
        same(out[0].cpu().numpy(), w_ptr, f"replay {which}: out_ptr")
        same(out[1].cpu().numpy()[:m], w_col, f"replay {which}: out_col")
        same(out[2].cpu().numpy()[:m], w_eid, f"replay {which}: out_eid")
        assert tuple(cout[2].tolist()) == w_counts
        same(cout[0].cpu().numpy()[:w_counts[0]], w_src, f"replay {which}: src_ids")
        same(cout[1].cpu().numpy(), w_local, f"replay {which}: local_col")
        # equal to the eager call on the same seeds
        e_ptr, e_col, e_eid = ops.sample_neighbors(ptr_d, idx_d, seeds_d, fanout, seed)
        assert torch.equal(e_ptr, out[0]) and torch.equal(e_eid[:m], out[2][:m])


# ------------------------------------------------------------------ 5. aggregation, autograd
POW2 = np.array([0.25, 0.5, 1.0, 2.0], np.float32)


@functools.lru_cache(maxsize=None)
def exact_block(name, fanout):
    """A block of the graph `name` as numpy arrays with power-of-two edge values."""
    ptr, idx, num_cols = sp.GRAPHS[name]()
    seeds = sp.seed_sets(ptr)["permutation"][:250]
    if name == "square":      # the hub row is one of the seeds
        seeds = np.unique(np.append(seeds, sp.hub_row(ptr)))[::-1].astype(np.int32).copy()
    b = sp.block_ref(ptr, idx, num_cols, seeds, fanout, seed=31)
    b["val"] = np.random.default_rng(4).choice(POW2, b["eid"].size)
    b["seeds"], b["name"] = seeds, name
    return b


def device_block(b, dev):
    """The mk.Block of a numpy block, through the library's own sampler: equal to the
    restatement, which is asserted."""
    parent_val = np.zeros(sp.GRAPHS[b["name"]]()[1].size, np.float32)
    parent_val[b["eid"]] = b["val"]
    g = csr_graph(b["name"], dev, dev_of(parent_val, dev))
    fanout = -1 if b.get("fanout") is None else b["fanout"]
    blk = mk.to_block(g, dev_of(b["seeds"], dev), fanout, 31)
    same(blk.ptr.cpu().numpy(), b["ptr"], "block ptr")
    same(blk.idx.cpu().numpy(), b["col"], "block idx")
    same(blk.eids.cpu().numpy(), b["eid"], "block eids")
    same(blk.src_ids.cpu().numpy(), b["src_ids"], "block src_ids")
    same(blk.val.cpu().numpy(), b["val"], "block val")
    assert blk.num_src == b["num_src"] and blk.num_dst == b["num_dst"]
    assert torch.equal(blk.dst_ids.cpu(), torch.from_numpy(b["seeds"]))
    return blk


def get_block(name, fanout, dev):
    b = dict(exact_block(name, fanout))
    b["fanout"] = fanout
    return b, device_block(b, dev)


AGG_SHAPES = ((256, 16), (64, 8), (100, 10))


@pytest.mark.parametrize("D,k", AGG_SHAPES)
@pytest.mark.parametrize("name,fanout", [("square", -1), ("rect", 10)])
def test_block_aggregation_is_exact_on_summable_inputs(gpu, name, fanout, D, k):
    """Features and gradients are multiples of 0.5 in [-4, 4] and the edge values powers of two:
    every sum is exact in f32, so the forward and x.grad equal the float64 dense restatement
    A_block @ densify(MaxK(x)) exactly (== on the values: bit for bit but for the sign of a
    zero)."""
    b, blk = get_block(name, fanout, gpu)
    ns, nd = b["num_src"], b["num_dst"]
    x = sp.exact_features(ns, D, seed=D + k)
    g_agg, g_self = gh.exact_grad(nd, D, seed=1), gh.exact_grad(nd, D, seed=2)
    A = sp.dense_block(b["ptr"], b["col"], b["val"], ns)
    xm, mask = sp.maxk_dense64(x, k)
    want_agg = A @ xm
    want_gx = mask * (A.T @ g_agg.astype(np.float64))
    want_gx_self = want_gx.copy()
    want_gx_self[:nd] += mask[:nd] * g_self

    xd = dev_of(x, gpu).requires_grad_(True)
    out = mk.block_aggregate(xd, blk, k)
    out.backward(dev_of(g_agg, gpu))
    same(out.detach().cpu().numpy(), want_agg.astype(np.float32), "block_aggregate")
    same(xd.grad.cpu().numpy(), want_gx.astype(np.float32), "block_aggregate: x.grad")

    xd = dev_of(x, gpu).requires_grad_(True)
    x_masked, agg = mk.block_self_aggregate(xd, blk, k)
    assert x_masked.shape == (ns, D) and agg.shape == (nd, D)
    (agg * dev_of(g_agg, gpu)).sum().add((x_masked[:nd] * dev_of(g_self, gpu)).sum()).backward()
    same(x_masked.detach().cpu().numpy(), xm.astype(np.float32), "x_masked")
    same(agg.detach().cpu().numpy(), want_agg.astype(np.float32), "block_self_aggregate")
    same(xd.grad.cpu().numpy(), want_gx_self.astype(np.float32), "block_self_aggregate: x.grad")


@pytest.mark.parametrize("D,k", AGG_SHAPES)
def test_block_aggregation_is_within_the_derived_bound(gpu, D, k):
    """Real inputs and mean weights: within (m + 4) u sum |terms| of the exact sum of the
    products of the f32 inputs, the bound the multi-head kernels guarantee (include/maxk_hip.h)."""
    b, blk = get_block("square", 25, gpu)
    blk = blk.with_values("mean")
    val = sp.block_values(b["ptr"], "mean")
    same(blk.val.cpu().numpy(), val, "mean values over the sampled edges")
    rng = np.random.default_rng(D)
    x = rng.standard_normal((b["num_src"], D)).astype(np.float32)
    g = rng.standard_normal((b["num_dst"], D)).astype(np.float32)
    xd = dev_of(x, gpu).requires_grad_(True)
    sp_data, sp_index = mk.maxk(xd, k)
    out = mk.block_spgemm(sp_data, sp_index, blk, D)
    sp_data.retain_grad()
    out.backward(dev_of(g, gpu))
    data, sel = sp_data.detach().cpu().numpy(), sp_index.cpu().numpy()
    ref, mag, m = gh.forward64(b["ptr"], b["col"], val[None], data, sel, D)
    err = np.abs(out.detach().cpu().numpy().astype(np.float64) - ref)
    assert (err <= gh.bound(mag, m)).all(), float((err / np.maximum(gh.bound(mag, m), 1e-300)).max())
    (gsp, gmag, gm), _ = gh.backward64(b["ptr"], b["col"], val[None], g, data, sel, D)
    gerr = np.abs(sp_data.grad.cpu().numpy().astype(np.float64) - gsp)
    assert (gerr <= gh.bound(gmag, gm)).all()
    print(f"\n  D={D} k={k}: worst forward err/bound "
          f"{float((err / np.maximum(gh.bound(mag, m), 1e-300)).max()):.3f}, backward "
          f"{float((gerr / np.maximum(gh.bound(gmag, gm), 1e-300)).max()):.3f}")
    # block_aggregate is the same two steps
    same(mk.block_aggregate(xd.detach(), blk, k).cpu().numpy(), out.detach().cpu().numpy(),
         "block_aggregate vs maxk + block_spgemm")


def test_a_blocks_plan_is_rectangular(gpu):
    """Block.plan() passes num_cols: the plan kernels on a block give the same exact sums."""
    D, k = 64, 8
    b, blk = get_block("rect", 10, gpu)
    ns, nd = b["num_src"], b["num_dst"]
    assert ns > nd
    plan = blk.plan(D, k)
    info = plan.info()
    assert (info["num_nodes"], info["num_cols"], info["num_edges"]) == (nd, ns, b["eid"].size)
    assert blk.plan(D, k) is plan
    x = sp.exact_features(ns, D, seed=6)
    g = gh.exact_grad(nd, D, seed=7)
    A = sp.dense_block(b["ptr"], b["col"], b["val"], ns)
    xm, _ = sp.maxk_dense64(x, k)
    data, sel = ops.maxk_forward(dev_of(x, gpu), k, return_index=True)
    same(plan.forward(data, sel).cpu().numpy(), (A @ xm).astype(np.float32), "plan forward")
    want = np.take_along_axis(A.T @ g.astype(np.float64), sel.cpu().numpy().astype(np.int64), 1)
    same(plan.backward(dev_of(g, gpu), sel).cpu().numpy(), want.astype(np.float32),
         "plan backward")


def test_autograd_drivers(gpu):
    """Twice through one graph, accumulation into .grad, and create_graph=True refused as
    elsewhere (the backwards are first order only)."""
    D, k = 64, 8
    b, blk = get_block("rect", 10, gpu)
    ns, nd = b["num_src"], b["num_dst"]
    x = sp.exact_features(ns, D, seed=9)
    g1, g2 = gh.exact_grad(nd, D, seed=3), gh.exact_grad(nd, D, seed=4)
    A = sp.dense_block(b["ptr"], b["col"], b["val"], ns)
    _, mask = sp.maxk_dense64(x, k)
    gx = lambda g: (mask * (A.T @ g.astype(np.float64))).astype(np.float32)  # noqa: E731

    xd = dev_of(x, gpu).requires_grad_(True)
    out = mk.block_aggregate(xd, blk, k)
    out.backward(dev_of(g1, gpu), retain_graph=True)
    same(xd.grad.cpu().numpy(), gx(g1), "first backward")
    out.backward(dev_of(g2, gpu))                      # the same graph again: accumulates
    same(xd.grad.cpu().numpy(), gx(g1) + gx(g2), "second backward through one graph")
    out2 = mk.block_aggregate(xd, blk, k)              # a second forward on the same block
    out2.backward(dev_of(g1, gpu))
    same(xd.grad.cpu().numpy(), gx(g1) + gx(g2) + gx(g1), "accumulated over two forwards")
    # used twice in one graph
    xd = dev_of(x, gpu).requires_grad_(True)
    (mk.block_aggregate(xd, blk, k) * dev_of(g1, gpu)).sum().add(
        (mk.block_aggregate(xd, blk, k) * dev_of(g2, gpu)).sum()).backward()
    same(xd.grad.cpu().numpy(), gx(g1) + gx(g2), "two uses in one graph")
    # no gradient asked for: nothing to run
    assert not mk.block_aggregate(xd.detach(), blk, k).requires_grad
    xd = dev_of(x, gpu).requires_grad_(True)
    (grad,) = torch.autograd.grad(mk.block_aggregate(xd, blk, k).sum(), xd, create_graph=True)
    with pytest.raises(RuntimeError):
        grad.sum().backward()


# ------------------------------------------------------------------ 6. layer and model
def norm_rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm().clamp(min=1e-30))


@pytest.mark.parametrize("agg", ["mean", "sum"])
@pytest.mark.parametrize("variant", ["maxk", "relu", "after_fc", "fused_dropout"])
def test_layer_on_the_full_block_equals_the_layer_on_the_graph(gpu, agg, variant):
    """fanout -1 and every row as a seed: the block is the graph, so the layer on it equals the
    layer on the CSRGraph up to the summation order (1e-5 norm-wise, the existing layers'
    tolerance), forward and parameter gradients."""
    graph = csr_graph("square", gpu)
    n = graph.num_nodes
    blk = mk.to_block(graph, torch.arange(n, dtype=torch.int32, device=gpu), -1, 3)
    assert blk.num_src == n == blk.num_dst and torch.equal(blk.idx, graph.idx)
    assert torch.equal(blk.ptr, graph.ptr)
    fin, fout, k = 64, 48, 8
    torch.manual_seed(5)
    kw = dict(maxk=k, nonlinear="relu" if variant == "relu" else "maxk",
              maxk_after_fc=variant == "after_fc")
    if variant == "fused_dropout":
        kw.update(feat_drop=0.3, fused_dropout=True)
    if variant == "after_fc":
        fout = 64
    layer = mk.MaxKSAGEConv(fin, fout, agg, **kw).to(gpu)
    x = torch.randn(n, fin, device=gpu)
    g = torch.randn(n, fout, device=gpu)
    res = []
    for gr in (graph, blk):
        layer.zero_grad()
        torch.manual_seed(77)                  # the fused dropout draws its seed from torch
        xin = x.clone().requires_grad_(True)
        out = layer(gr, xin)
        out.backward(g)
        res.append((out, xin.grad, [p.grad.clone() for p in layer.parameters()]))
    (o_g, x_g, p_g), (o_b, x_b, p_b) = res
    assert o_b.shape == (n, fout)
    worst = max([norm_rel(o_b, o_g), norm_rel(x_b, x_g)] +
                [norm_rel(a, b) for a, b in zip(p_b, p_g)])
    print(f"\n  {agg} {variant}: worst norm-wise difference {worst:.2e}")
    assert worst <= 1e-5, worst


def test_two_layer_sage_over_the_sampler_matches_float64(gpu):
    """MaxKSAGE over NeighborSampler([5, 5]) against a dense float64 restatement built from the
    blocks. The restatement takes each layer's top-k mask from the f32 input the layer saw (a
    mask is a discrete function of it) and computes everything else in float64; the f32 model
    then differs by the rounding of four matrix products of inner size <= 64 and two
    aggregations of <= 5 terms: 1e-5 norm-wise, the layers' tolerance."""
    graph = csr_graph("square", gpu)
    ptr, idx, num_cols = sp.square_graph()
    seeds = sp.seed_sets(ptr)["permutation"][:128]
    sampler = mk.NeighborSampler([5, 5], seed=12)
    input_ids, output_ids, blocks = sampler.sample(graph, dev_of(seeds, gpu))
    assert sampler.calls == 1 and len(blocks) == 2
    # the blocks are the restated ones, inner seeds = the outer block's src_ids
    b1 = sp.block_ref(ptr, idx, num_cols, seeds, 5, mk.layer_seed(12, 0, 1))
    b0 = sp.block_ref(ptr, idx, num_cols, b1["src_ids"], 5, mk.layer_seed(12, 0, 0))
    for blk, ref in zip(blocks, (b0, b1)):
        same(blk.ptr.cpu().numpy(), ref["ptr"], "sampler block ptr")
        same(blk.idx.cpu().numpy(), ref["col"], "sampler block idx")
        same(blk.src_ids.cpu().numpy(), ref["src_ids"], "sampler block src_ids")
        same(blk.eids.cpu().numpy(), ref["eid"], "sampler block eids")
    same(output_ids.cpu().numpy(), seeds, "output_ids")
    same(input_ids.cpu().numpy(), b0["src_ids"], "input_ids")
    assert torch.equal(blocks[0].dst_ids, blocks[1].src_ids)
    # a second call draws other blocks; a new sampler with the same seed replays the first
    again = sampler.sample(graph, dev_of(seeds, gpu))[2]
    assert not torch.equal(again[1].eids, blocks[1].eids)
    replay = mk.NeighborSampler([5, 5], seed=12).sample(graph, dev_of(seeds, gpu))[2]
    assert all(torch.equal(a.eids, b.eids) for a, b in zip(replay, blocks))

    fin, hid, classes, k = 32, 64, 7, 8
    torch.manual_seed(8)
    model = mk.MaxKSAGE(fin, hid, 2, classes, maxk=k, feat_drop=0.0).to(gpu).eval()
    feats = torch.randn(num_cols, fin, device=gpu)
    seen = []
    hooks = [layer.register_forward_pre_hook(lambda mod, args: seen.append(args[1].detach()))
             for layer in model.layers]
    x = feats[input_ids.long()].requires_grad_(True)
    out = model(blocks, x)
    for h in hooks:
        h.remove()
    assert out.shape == (len(seeds), classes) and len(seen) == 2

    def w(t):
        return t.detach().double().cpu().numpy()

    h = w(x) @ w(model.lin_in.weight).T + w(model.lin_in.bias)
    for layer, ref, inp in zip(model.layers, (b0, b1), seen):
        _, mask = sp.maxk_dense64(inp.cpu().numpy(), k)
        xm = h * mask
        A = sp.dense_block(ref["ptr"], ref["col"], sp.block_values(ref["ptr"], "mean"),
                           ref["num_src"])
        h = (xm[:ref["num_dst"]] @ w(layer.fc_self.weight).T +
             (A @ xm) @ w(layer.fc_neigh.weight).T + w(layer.bias))
    want = h @ w(model.lin_out.weight).T + w(model.lin_out.bias)
    rel = float(np.linalg.norm(w(out) - want) / np.linalg.norm(want))
    print(f"\n  two-layer MaxKSAGE on sampled blocks: norm-wise difference {rel:.2e}")
    assert rel <= 1e-5, rel
    # and it trains: a step moves the parameters
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    loss = model(blocks, x.detach()).square().mean()
    loss.backward()
    before = [p.detach().clone() for p in model.parameters()]
    opt.step()
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))


# ------------------------------------------------------------------ 7. scan lengths
@pytest.mark.parametrize("n", scan.LENGTHS)
def test_sampler_scans_n_items(gpu, n):
    """out_ptr is scanned over S + 1 = n items: S seeds drawn with repetition from the 300-row
    graph, every neighbour kept, so out_ptr is the cumulative sum of the seeds' row lengths and
    out_eid the concatenation of their edge ranges."""
    ptr, idx, _ = sp.rect_graph()
    ptr_d, idx_d, _ = graph_dev("rect", gpu)
    seeds = np.random.default_rng(n).integers(0, ptr.size - 1, n - 1).astype(np.int32)
    lens = np.diff(ptr).astype(np.int64)[seeds]
    w_ptr = np.zeros(n, np.int64)
    np.cumsum(lens, out=w_ptr[1:])
    m = int(w_ptr[-1])
    assert m < 2 ** 31
    w_eid = np.arange(m) + np.repeat(ptr[seeds] - w_ptr[:-1], lens)
    out = tuple(torch.full((size,), -7, dtype=torch.int32, device=gpu) for size in (n, m, m))
    ops.sample_neighbors(ptr_d, idx_d, dev_of(seeds, gpu), -1, 3, out=out)
    same(out[0].cpu().numpy(), w_ptr.astype(np.int32), f"{n} items: out_ptr")
    same(out[2].cpu().numpy(), w_eid.astype(np.int32), f"{n} items: out_eid")
    same(out[1].cpu().numpy(), idx[w_eid], f"{n} items: out_col")
    if seeds.size:
        COVERED.update(sampler_names(-1))


@pytest.mark.parametrize("n", scan.LENGTHS)
def test_compaction_scans_n_columns(gpu, n):
    """The new columns are counted and placed over num_cols = n items: 300 seeds (below the last
    column where there is more than one), 3,000 sampled columns over the whole range with the
    first column, the last one and a seed among them."""
    rng = np.random.default_rng(n)
    seeds = rng.choice(max(n - 1, 1), min(300, max(n - 1, 1)), replace=False).astype(np.int32)
    cols = rng.integers(0, n, 3000).astype(np.int32)
    cols[:3] = (n - 1, 0, seeds[0])
    w_src, w_local, w_counts = sp.compact_ref(seeds, cols, n)
    assert n == 1 or w_src[-1] == n - 1          # the last column is a new one, placed last
    src, local, counts = ops.block_compact(dev_of(seeds, gpu), dev_of(cols, gpu), n)
    assert tuple(counts.tolist()) == w_counts, n
    same(src.cpu().numpy()[:w_counts[0]], w_src, f"{n} columns: src_ids")
    same(local.cpu().numpy(), w_local, f"{n} columns: local_col")
    COVERED.update(sp.COMPACT_KERNELS)


# ------------------------------------------------------------------ 8. closure (keep last)
def test_every_sampler_instantiation_was_launched_by_a_passing_case(gpu):
    names = compiled()
    assert len(names) == 7 + len(sp.SCAN_KERNELS) == 12
    missing = sorted(names - COVERED)
    assert not missing, f"instantiations without a passing case: {missing}"
    assert not COVERED - names
