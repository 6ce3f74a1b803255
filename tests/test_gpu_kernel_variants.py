"""GPU: one checked launch per compiled kernel instantiation.

For every name of tests/golden/kernel_instantiations.txt (what tools/kernel_list.py reads from
the built library) tests/kernel_variants.py holds at least one case: a graph, k, D, options and
entry point built to launch that instantiation. Each case

1. asserts that the dispatch restated in tests/kernel_variants.py names the targeted
   instantiation for the plan's info() and the call's arguments,
2. runs the kernel on exactly summable inputs (the sweep's graphs and recipe), and
3. compares bit for bit with the oracle's f64 sums or the numpy restatements of the *_capi tests.

The last test is the closure: the targets of the cases that ran equal the fixture's set, with no
exemption (under a -k selection it skips). Run with -s for the cases per kernel family, their
wall time and the slowest case.

The four kernels for grad_out above 4 GiB run on a 4,194,344 x 300 plan whose few thousand edges
sit in the first rows, on both sides of the 4 GiB boundary and in the last rows; grad_out is a
zero-filled 4.3 GB device buffer of which only those rows are written.
"""
import collections
import functools
import time

import numpy as np
import pytest
import torch

import kernel_variants as kv
import maxk_kernels as mk
from maxk_kernels import ops
import rowconst
import sweep
from oracle import oracle
from structured import int_features
from test_dropout_capi import dropped_table
from test_edge_grad_capi import edge_grad_rows
from test_gat_attention_capi import transposed
from test_gpu_contracts import stats_pair
from test_gpu_parity import to_dev
from test_gpu_records import SENTINEL, pack_records
from test_gpu_sweep import assert_bits, assert_exact, dev_case, dev_graph
from test_self_capi import dense_rows, merge_rows

pytestmark = pytest.mark.gpu

N, D = sweep.N, sweep.D_FULL
DROP = (sweep.DROP_P, sweep.SEED, sweep.ROW_OFFSET)
CASES = kv.cases()
COVERED = collections.defaultdict(list)       # target -> ids of the cases that passed
SECONDS = {}                                  # case id -> wall seconds
STARTED = set()                               # ids of the cases that began


# ------------------------------------------------------------------ plans
def exact_plan(gpu, gname, k, opts):
    """(plan, case, rows, columns) on one of the sweep's graphs or rowconst's tiles graph."""
    if gname == "tiles":
        c = rowconst.exact_case("tiles", k)
        ptr, idx, val = to_dev(c.p, gpu), to_dev(c.ix, gpu), to_dev(c.v, gpu)
        plan = mk.GraphPlan(ptr, idx, val, c.n, c.ix.size, D, k, num_cols=rowconst.NCOLS,
                            options=opts)
        return plan, c, c.n, rowconst.NCOLS
    c = sweep.case(gname, D, k)
    ptr, idx, val = dev_graph(gpu, gname)
    return mk.GraphPlan(ptr, idx, val, N, c.ix.size, D, k, options=opts), c, N, N


def check_forward(gpu, plan, c, what):
    ref = c.ref if hasattr(c, "ref") else c.fwd
    assert_exact(plan.forward(to_dev(c.od, gpu), to_dev(c.oi, gpu)), ref, what + " forward")


def run_forward(gpu, case):
    p = case.p
    plan, c, _, _ = exact_plan(gpu, p["graph"], p["k"], p["opts"])
    info = plan.info()
    if case.family == "forward":
        assert kv.forward_kernel(info) == case.target, (case.id, info)
    else:
        assert case.target in kv.forward_pass_kernels(info), (case.id, info)
    check_forward(gpu, plan, c, case.id)


def run_column_blocks(gpu, case):
    p = case.p
    plan, c, n, nc = exact_plan(gpu, p["graph"], p["k"], p["opts"])
    info = plan.info()
    assert info["bwd_algo"] == 1, (case.id, info)
    f, s, kp = kv.bwd_slots(p["k"], p["opts"], n, nc, c.ix.size)
    assert kv.column_block_kernel(info, f, s, kp) == case.target, (case.id, info, f, s, kp)
    _, oi, g = dev_case(gpu, p["graph"], D, p["k"])
    assert_exact(plan.backward(g, oi), c.bwd, case.id + " backward")


def run_bwd_big(gpu, case):
    k, opts = case.p["k"], case.p["opts"]
    c = kv.big_case(k)
    assert c.n * D * 4 > 2 ** 32
    torch.cuda.empty_cache()
    ptr, idx, val = to_dev(kv.big_ptr(c), gpu), to_dev(c.ix, gpu), to_dev(c.v, gpu)
    plan = mk.GraphPlan(ptr, idx, val, c.n, c.ix.size, D, k, num_cols=c.nc, options=opts)
    info = plan.info()
    assert info["bwd_algo"] == 1 and (info["bwd_waves"], info["bwd_unroll"]) == (8, 8), info
    f, s, kp = kv.bwd_slots(k, opts, c.n, c.nc, c.ix.size)
    assert kv.column_block_kernel(info, f, s, kp) == case.target, (case.id, info, f, s, kp)
    g = torch.zeros((c.n, D), dtype=torch.float32, device=gpu)
    g[to_dev(c.rows, gpu)] = to_dev(c.g, gpu)
    gs = plan.backward(g, to_dev(c.oi, gpu))
    torch.cuda.synchronize()
    try:
        assert_exact(gs, c.bwd, case.id + " backward")
    finally:
        del plan, g, gs
        torch.cuda.empty_cache()


def run_row_pass(gpu, case):
    c = kv.tp_case(case.p["deg"])
    ptr, idx, val = to_dev(c.p, gpu), to_dev(c.ix, gpu), to_dev(c.v, gpu)
    plan = mk.GraphPlan(ptr, idx, val, c.n, c.ix.size, D, c.k, num_cols=c.nc,
                        options=case.p["opts"])
    info = plan.info()
    assert info["bwd_algo"] == 3, (case.id, info)
    assert kv.row_pass_kernel(c.n, c.ix.size) == case.target, case.id
    assert_exact(plan.backward(to_dev(c.g, gpu), to_dev(c.oi, gpu)), c.bwd, case.id + " backward")


# ------------------------------------------------------------------ top-k, scatter
@functools.lru_cache(maxsize=8)
def topk_ref(d, k, mode):
    x = sweep.topk_rows(d)
    od, oi = oracle.maxk(x, k, mode)
    return x, od, oi, sweep.topk_counts(x, k, mode)


def run_topk(gpu, case):
    p = case.p
    mode, n, d, k = p["mode"], p["n"], p["d"], p["k"]
    assert kv.topk_kernel(**p) == case.target, case.id
    x, od, oi, cnt = topk_ref(d, k, mode)
    if n >= kv.TOPK_ROWS8:                     # the 40 rows repeated: compared on the device
        reps = -(-n // 40)
        xt = to_dev(x, gpu).repeat(reps, 1)[:n].contiguous()
        sd, si = mk.maxk_forward(xt, k, mode=mode, return_index=True)
        want_d = to_dev(od, gpu).view(torch.int32).repeat(reps, 1)[:n]
        want_i = to_dev(oi, gpu).repeat(reps, 1)[:n]
        assert torch.equal(si, want_i), case.id + " selectors"
        assert torch.equal(sd.view(torch.int32), want_d), case.id + " values"
        del xt, sd, si, want_d, want_i
        torch.cuda.empty_cache()
        return
    rows = sweep.TOPK_FINITE if p["stats"] else 40       # the statistics take finite rows
    table = dropped_table(od, oi, *DROP) if p["dropout"] else od
    table, oi, cnt = table[:rows], oi[:rows], cnt[:rows]
    kw = dict(mode=mode, return_index=True, return_count=True)
    if p["stats"]:
        kw["stats"] = torch.full((2,), -1, dtype=torch.int32, device=gpu)
    if p["dropout"]:
        kw["dropout"] = DROP
    if p["records"]:
        layout = 1 if k > kv.WAVE else 4          # packed records at k = 72, pair chunks at 16
        rb = (sweep.record_chunk_bytes(layout, k) + 15) // 16 * 16 + 32
        rec = torch.full((rows, rb), SENTINEL, dtype=torch.uint8, device=gpu)
        kw["records"] = (rec, layout)
    if p["dense"]:
        kw["dense"] = torch.full((rows, d), float("nan"), device=gpu)
    sd, si, sc = mk.maxk_forward(to_dev(x[:rows], gpu), k, **kw)
    assert_bits(si, oi, case.id + " selectors")
    assert_bits(sd, table, case.id + " values")
    assert np.array_equal(sc.cpu().numpy(), cnt), case.id + " counts"
    if p["stats"]:
        assert kw["stats"].tolist() == stats_pair(table).tolist(), case.id + " statistics pair"
    if p["records"]:
        want = pack_records(torch.from_numpy(table), torch.from_numpy(oi), layout, rb).numpy()
        assert np.array_equal(rec.cpu().numpy(), want), case.id + " record bytes"
    if p["dense"]:
        assert_bits(kw["dense"], dense_rows(table, oi, cnt, d), case.id + " dense row")


def run_scatter(gpu, case):
    p = case.p
    k, d = p["k"], p["d"]
    assert kv.scatter_kernel(p["dropout"], p["merge"]) == case.target, case.id
    gs = int_features(40, k, seed=7300)
    gd = int_features(40, d, seed=7301)
    for mode in sweep.MODES:
        oi = topk_ref(d, k, mode)[2]
        got = mk.maxk_backward(to_dev(gs, gpu), to_dev(oi, gpu), dim_origin=d,
                               dropout=DROP if p["dropout"] else None,
                               grad_dense=to_dev(gd, gpu) if p["merge"] else None)
        if p["dropout"] or p["merge"]:
            ref = merge_rows(gs, oi, gd if p["merge"] else None,
                             *(DROP if p["dropout"] else (0.0, 0, 0)), D=d)
        else:
            ref = oracle.maxk_backward(gs, oi, d)
        assert_bits(got, ref, f"{case.id} {mode}")


def run_sddmm(gpu, case):
    k = case.p["k"]
    assert kv.sddmm_kernel(k) == case.target, case.id
    p, ix, _ = sweep.graph("sparse")
    ptr, idx, _ = dev_graph(gpu, "sparse")
    c = sweep.case("sparse", D, k)
    od, oi, g = dev_case(gpu, "sparse", D, k)
    got = mk.spgemm_edge_grad(ptr, idx, g, od, oi, N, ix.size, k, D)
    rows = np.repeat(np.arange(N), np.diff(p))
    f64 = (c.od[ix].astype(np.float64) * c.g[rows[:, None], c.oi[ix]]).sum(1)
    ref = edge_grad_rows(p, ix, c.g, c.od, c.oi)
    assert np.array_equal(ref, f64)
    assert_bits(got, ref, case.id)


def run_dense_spmm(gpu, case):
    d = case.p["d"]
    assert kv.dense_spmm_kernel(d) == case.target, case.id
    x, y, _ = kv.dense_spmm_case(d)
    ptr, idx, val = dev_graph(gpu, "sparse")
    assert_exact(mk.dense_spmm(ptr, idx, val, to_dev(x, gpu)), y, case.id)


# ------------------------------------------------------------------ single-instance kernels
def plan_scenario(gpu, name):
    gname, k, opts = kv.PLAN_SCENARIOS[name]
    plan, c, _, _ = exact_plan(gpu, gname, k, opts)
    info = plan.info()
    check_forward(gpu, plan, c, name)
    _, oi, g = dev_case(gpu, gname, D, k)
    assert_exact(plan.backward(g, oi), c.bwd, name + " backward")
    if name in ("identity_order", "scattered"):
        order = mk.plan_col_order(plan).cpu().numpy()
        assert np.array_equal(np.sort(order), np.arange(N)), name + ": not a permutation"
        assert np.array_equal(order, np.arange(N)) == (name == "identity_order"), name
    return dict(info=info, opts=opts)


def value_refresh(gpu):
    """Row-constant values at build, a refresh to mixed values, a refresh back: the forward after
    each against the oracle."""
    k = kv.REFRESH_K
    const, mixed = rowconst.exact_case("tiles", k), rowconst.exact_case("tiles", k, break_row=5)
    ptr, idx, val = to_dev(const.p, gpu), to_dev(const.ix, gpu), to_dev(const.v, gpu)
    plan = mk.GraphPlan(ptr, idx, val, const.n, const.ix.size, D, k, num_cols=rowconst.NCOLS)
    seen = []
    for step, c in enumerate((const, mixed, const)):
        if step:
            val.copy_(to_dev(c.v, gpu))
            plan.refresh_values(val)
        seen.append(plan.info()["fwd_rowconst"])
        check_forward(gpu, plan, c, f"value_refresh step {step}")
    return dict(rowconst=seen)


def stats_odd_k(gpu):
    k = kv.STATS_ODD_K
    c = sweep.case("sparse", D, k)
    st = mk.cbsr_stats(to_dev(c.od, gpu), to_dev(c.oi, gpu))
    assert st.view(-1).tolist() == stats_pair(c.od).tolist()
    return dict(k=k)


def topk_count(gpu):
    x, od, oi, _ = topk_ref(D, 16, "exact")
    fin = sweep.TOPK_FINITE
    st = torch.full((2,), -1, dtype=torch.int32, device=gpu)
    sd, sc = mk.maxk_forward(to_dev(x[:fin], gpu), 16, return_count=True, stats=st)
    assert sc.tolist() == [16] * fin
    assert st.tolist() == stats_pair(od[:fin]).tolist()
    assert_bits(sd, od[:fin], "topk_count values")
    return dict(mode="exact", count=True, stats=True)


def edge_softmax(gpu):
    c = kv.attention_case()
    gl = kv.attention_refs(c)[0]
    ptr = to_dev(c.ptr, gpu)
    assert_exact(ops.edge_softmax(ptr, to_dev(c.logits, gpu)), c.alpha, "edge_softmax")
    assert_exact(ops.edge_softmax_backward(ptr, to_dev(c.alpha, gpu), to_dev(c.ga, gpu)), gl,
                 "edge_softmax_backward")
    return {}


def gat_attention(gpu):
    c = kv.attention_case()
    _, ge, ger, gel = kv.attention_refs(c)
    ptr, idx, el, er = (to_dev(a, gpu) for a in (c.ptr, c.idx, c.el, c.er))
    alpha = ops.gat_attention(ptr, idx, el, er, kv.ATT_SLOPE)
    assert_exact(alpha, c.alpha, "gat_attention")
    got_e, got_er = ops.gat_attention_backward(ptr, idx, el, er, kv.ATT_SLOPE, alpha,
                                              to_dev(c.ga, gpu))
    assert_exact(got_e, ge, "gat_attention_backward grad_edge")
    assert_exact(got_er, ger, "gat_attention_backward grad_er")
    ptr_t, order = transposed(c.idx, c.nc)
    assert_exact(ops.edge_colsum(to_dev(ptr_t, gpu), to_dev(order, gpu), got_e), gel,
                 "edge_colsum")
    return {}


OTHER_SCENARIOS = dict(value_refresh=value_refresh, stats_odd_k=stats_odd_k,
                       topk_count=topk_count, edge_softmax=edge_softmax,
                       gat_attention=gat_attention)


@functools.lru_cache(maxsize=None)
def scenario(gpu, name):
    """The facts of a scenario that ran and passed its checks (once per session)."""
    if name in kv.PLAN_SCENARIOS:
        return plan_scenario(gpu, name)
    return OTHER_SCENARIOS[name](gpu)


def run_single(gpu, case):
    name, _, shows = kv.SINGLES[case.target]
    facts = scenario(gpu, name)
    assert shows(facts), (case.id, kv.SINGLES[case.target][1], facts)


RUNNERS = dict(forward=run_forward, forward_pass=run_forward, column_blocks=run_column_blocks,
               bwd_big=run_bwd_big, row_pass=run_row_pass, topk=run_topk, scatter=run_scatter,
               sddmm=run_sddmm, dense_spmm=run_dense_spmm, single=run_single)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_instantiation(gpu, case):
    STARTED.add(case.id)
    t0 = time.perf_counter()
    RUNNERS[case.family](gpu, case)
    torch.cuda.synchronize()
    SECONDS[case.id] = time.perf_counter() - t0
    COVERED[case.target].append(case.id)


# ------------------------------------------------------------------ the closure
EXEMPT = set()                                # instantiations no case reaches: none


def test_every_instantiation_ran(gpu):
    """Runs last (file order): the targets of the cases that passed are exactly the fixture's
    names. Skips under a -k selection; in a whole-module run every case must have run."""
    if len(STARTED) < len(CASES):
        pytest.skip(f"a selection ran {len(STARTED)} of {len(CASES)} cases")
    names = set(kv.fixture_names())
    missing = sorted(names - set(COVERED) - EXEMPT)
    extra = sorted(set(COVERED) - names)
    assert not missing, f"{len(missing)} instantiations without a passing case: {missing}"
    assert not extra, f"cases target names the library does not hold: {extra}"
    assert not EXEMPT
    fam = collections.defaultdict(lambda: [0, set(), 0.0])
    for c in CASES:
        fam[c.family][0] += 1
        fam[c.family][1].add(c.target)
        fam[c.family][2] += SECONDS.get(c.id, 0.0)
    print(f"\nkernel variants: {len(CASES)} cases launched {len(COVERED)} of {len(names)} "
          f"instantiations in {sum(SECONDS.values()):.1f} s")
    for name, (n, targets, sec) in fam.items():
        print(f"  {name}: {n} cases, {len(targets)} instantiations, {sec:.1f} s")
    slow = max(SECONDS, key=SECONDS.get)
    print(f"  slowest case: {slow} {SECONDS[slow]:.2f} s")
