"""GPU parity on structured inputs (tests/structured.py; their preconditions are checked on the
CPU in tests/test_structured_inputs.py):

A. exactly summable data (integer features, edge values in {0.5, 1, 2}) on hub-column graphs:
   every kernel must equal the f64 oracle bit for bit as floats, whatever the order of its
   sums, so one lost, doubled or misplaced update fails whatever the in-degree;
B. the f32 backward on hub columns with inexact same-sign terms, against the 1e-5 bar where a
   running f32 sum keeps it and against the f32 summation bound beyond (figures printed with
   the prefix "structured-B", kept in profiles/r09/structured_inputs.log);
C. wide edge-value and feature ranges through the forward's per-task fixed-point decision;
D. NaN and +-Inf in edge values, tables and gradients against the oracle's IEEE sums.
"""
import numpy as np
import pytest
import torch

import maxk_kernels as mk
import structured as st
from oracle import oracle
from test_gpu_parity import graph_on, to_dev

pytestmark = pytest.mark.gpu


def ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def plan_for(gpu, c, d, k, opts):
    ptr, idx, val = graph_on(gpu, c.p, c.ix, c.v)
    return mk.GraphPlan(ptr, idx, val, c.n, c.ix.size, d, k, options=opts)


def assert_equal_floats(got, ref, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    ref = np.asarray(ref).astype(np.float32)
    bad = got != ref
    assert got.shape == ref.shape and not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at "
        f"{tuple(int(i) for i in np.argwhere(bad)[0])}: got {got[bad][:4]}, oracle {ref[bad][:4]}")
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------ A: exact
EXACT_CASES = [(g, d, k) for g in st.EXACT_GRAPHS for d, k in st.EXACT_DK]
TWO_PASS_K = (8, 16, 32, 64)        # k / 4 a power of two: the two-pass backward's range
# the column-block options are forced onto the block kernel (bwd_algo=1): the defaults take the
# two-pass form on the star at k >= 32, which ignores them. plan.info() reports neither the
# slots per lane nor the flush, so those two cases show only that they ran the block kernel
BWD_OPTS = [dict(), dict(bwd_algo=1), dict(bwd_algo=1, bwd_features_per_lane=2),
            dict(bwd_algo=1, bwd_flush=1), dict(bwd_algo=1, bwd_piece_edges=500),
            dict(bwd_algo=1, bwd_handout=1),
            # two slot groups double the block's columns: the default cap no longer cuts the
            # star's hub block at k <= 8, so the cap is set
            dict(bwd_algo=1, bwd_slot_groups=2, bwd_piece_edges=8192), dict(bwd_algo=3)]
FWD_OPTS = [dict(), dict(fwd_fixed=2), dict(fwd_chunk3=3), dict(fwd_chunk3=1),
            dict(fwd_task_cap=512)]


@pytest.mark.parametrize("opts", FWD_OPTS, ids=ids)
@pytest.mark.parametrize("gname,d,k", EXACT_CASES)
def test_exact_forward(gpu, gname, d, k, opts):
    c = st.exact_case(gname, d, k)
    assert st.exactly_summable(c.fwd_mag)              # precondition on the inputs
    plan = plan_for(gpu, c, d, k, opts)
    info = plan.info()
    if gname == "star20000":                           # the hub rows are split into segments
        assert info["fwd_split_rows"] == 3
        if "fwd_task_cap" in opts:
            assert info["fwd_tasks"] >= 3 * (c.n // 512)
    if opts.get("fwd_fixed") == 2:
        assert info["fwd_fixed"] == 0
    elif k >= 16:
        assert info["fwd_fixed"] == 1
    if opts.get("fwd_chunk3") == 3:
        assert info["fwd_layout"] == (4 if k % 2 == 0 else 2)
    if opts.get("fwd_chunk3") == 1:
        assert info["fwd_layout"] == 2
    out = plan.forward(to_dev(c.od, gpu), to_dev(c.oi, gpu))
    assert_equal_floats(out, c.fwd, "forward")


def block_cols(n, slots):
    """Columns per backward block with `slots` accumulators per column: what the LDS budget
    holds, then 8 or more blocks rounded up to a multiple of the 8 XCDs (of 64 from 64 on)."""
    cols = min(n, (160 * 1024 - 16) // (5 * slots))
    blocks = -(-n // cols)
    if blocks >= 8:
        q = 64 if blocks >= 64 else 8
        cols = -(-n // (-(-blocks // q) * q))
    return cols


@pytest.mark.parametrize("opts", BWD_OPTS, ids=ids)
@pytest.mark.parametrize("gname,d,k", EXACT_CASES)
def test_exact_backward_and_scatter(gpu, gname, d, k, opts):
    c = st.exact_case(gname, d, k)
    assert st.exactly_summable(c.bwd_mag)              # precondition on the inputs
    plan = plan_for(gpu, c, d, k, opts)
    info = plan.info()
    if opts.get("bwd_algo") == 3:
        assert info["bwd_algo"] == (3 if k in TWO_PASS_K else 1)
    elif not opts:
        if gname == "star20000":     # 7 edges per row over 10 and 20 blocks: two-pass
            assert info["bwd_algo"] == (3 if k in (32, 64) else 1)
    else:
        assert info["bwd_algo"] == 1
        if gname == "star20000":                       # the hub block is cut into pieces
            assert info["bwd_shared_blocks"] > 0
        if "bwd_piece_edges" in opts:
            assert info["bwd_tasks"] >= c.ix.size // opts["bwd_piece_edges"]
        if "bwd_handout" in opts:
            assert info["bwd_handout"] == 1
        if "bwd_slot_groups" in opts:
            # a block holds (LDS budget - 16) / (5 x slots per group) columns, so two groups
            # show as twice the columns; k = 10 (two slots per lane, 10 % 4 != 0) cannot be
            # halved and runs one group
            slots = {16: 8, 8: 4, 32: 16, 64: 32, 7: 4, 10: 10}[k]
            assert info["bwd_block_cols"] == block_cols(c.n, slots)
    oi = to_dev(c.oi, gpu)
    gs = plan.backward(to_dev(c.g, gpu), oi)
    assert_equal_floats(gs, c.bwd, "backward")
    gin = mk.maxk_backward(gs, oi, dim_origin=d)
    assert_equal_floats(gin, oracle.maxk_backward(c.bwd, c.oi, d), "MaxK scatter")


@pytest.mark.parametrize("gname,d", [(g, d) for g in st.EXACT_GRAPHS for d in (256, 100)])
def test_exact_dense_spmm(gpu, gname, d):
    p, ix, v = st.exact_graph(gname)
    n = p.size - 1
    x = st.int_features(n, d, seed=3000 + d)
    assert st.exactly_summable(oracle.dense_spmm(p, ix, np.abs(v), np.abs(x)))
    a = torch.sparse_csr_tensor(torch.from_numpy(p).long(), torch.from_numpy(ix).long(),
                                torch.from_numpy(v).double(), size=(n, n))
    ref = (a @ torch.from_numpy(x).double()).numpy()   # f64 sums
    y = mk.dense_spmm(*graph_on(gpu, p, ix, v), to_dev(x, gpu))
    assert_equal_floats(y, ref, "dense SpMM")


@pytest.mark.parametrize("drop", [0.0, 0.5], ids=["plain", "dropout"])
@pytest.mark.parametrize("mode", ["exact", "ref_compat"])
@pytest.mark.parametrize("gname,d,k", EXACT_CASES)
def test_exact_aggregate_end_to_end(gpu, gname, d, k, mode, drop):
    """maxk_aggregate's output and x.grad: top-k (ties to the lowest index; with dropout the
    numpy mask's table, scale 2) -> forward -> backward -> scatter, all exact."""
    c = st.exact_case(gname, d, k, mode, drop)
    assert st.exactly_summable(c.fwd_mag, c.bwd_mag, c.gx_mag)
    graph = mk.CSRGraph(*graph_on(gpu, c.p, c.ix, c.v))
    x = to_dev(c.x, gpu).requires_grad_(True)
    y = mk.maxk_aggregate(x, graph, k, mode, dropout_p=drop, seed=st.EXACT_SEED)
    y.backward(to_dev(c.g, gpu))
    assert_equal_floats(y, c.fwd, "maxk_aggregate")
    assert_equal_floats(x.grad, c.gx, "x.grad")


# ------------------------------------------------------------------------------ B: hub sums
HUB_OPTS = [dict(), dict(bwd_algo=3), dict(bwd_flush=1)]


@pytest.mark.parametrize("opts", HUB_OPTS, ids=ids)
@pytest.mark.parametrize("name", list(st.HUB_CASES))
def test_hub_backward_same_sign_terms(gpu, name, opts):
    """Hub columns of in-degree 4,096 at the 1e-5 bar (a running f32 sum uses 0.14 of it,
    test_structured_inputs.py), of in-degree 16,385 at (n_c + 2) 2^-24 mag per element: random
    same-sign terms and the constant terms of y.sum().backward() through a sum aggregator."""
    c = st.hub_case(name)
    plan = plan_for(gpu, c, st.HUB_D, st.HUB_K, opts)
    if "bwd_algo" in opts:
        assert plan.info()["bwd_algo"] == 3
    got = plan.backward(to_dev(c.g, gpu), to_dev(c.oi, gpu)).cpu().numpy().astype(np.float64)
    err = np.abs(got - c.bwd.astype(np.float64))
    mag = c.bwd_mag.astype(np.float64)
    bar_ok, bar = oracle.close_enough(got, c.bwd, c.bwd_mag, rtol=st.RTOL)
    summ = float((err / st.summation_bound(c.ncol, mag)).max())
    print(f"structured-B backward {name} {ids(opts)} algo={plan.info()['bwd_algo']}: "
          f"worst err/(1e-5 bar) {bar:.3g}, worst err/((n_c+2) 2^-24 mag) {summ:.3g}, "
          f"worst |err|/mag {float((err / mag).max()):.3g}")
    if c.n == 4096:
        assert bar_ok, f"worst err / 1e-5 bar = {bar:.3g}"
    else:
        assert summ <= 1.0, f"worst err / summation bound = {summ:.3g}"


@pytest.mark.parametrize("fixed", [0, 2], ids=["fixed_point", "f64"])
@pytest.mark.parametrize("name", list(st.HUB_CASES))
def test_hub_forward_same_sign_terms(gpu, name, fixed):
    """The forward of the same graphs. It accumulates in fixed point or f64, so every row that is
    one task owes 2^-24 + 2^-23 relative. A hub row of 16,385 edges is split into 5 segments
    whose f32 sums are added with f32 atomics in an order the kernel does not fix, so it owes
    (segments + 2) 2^-24 (structured.split_row_bound). With the constant terms every order of
    those adds stays within 2.3 x 2^-24 on these arrays (enumerated in
    test_structured_inputs.py::test_split_hub_rows_every_order_of_the_segment_adds), so the
    constant cases keep 2^-24 + 2^-23 on the hub rows too."""
    c = st.hub_case(name)
    plan = plan_for(gpu, c, st.HUB_D, st.HUB_K, dict(fwd_fixed=fixed))
    info = plan.info()
    hubs = [0, 1, c.n - 1]
    split = c.n > st.FWD_TASK_CAP
    segments = -(-c.n // st.FWD_TASK_CAP)
    assert info["fwd_split_rows"] == (3 if split else 0)
    assert info["fwd_fixed"] == (1 if fixed == 0 else 0)
    out = plan.forward(to_dev(c.od, gpu), to_dev(c.oi, gpu)).cpu().numpy()
    whole = np.ones(c.n, bool)
    whole[hubs] = not split
    rel = oracle.worst_relative(out[whole], c.fwd[whole], c.fwd_mag[whole])
    hub = oracle.worst_relative(out[hubs], c.fwd[hubs], c.fwd_mag[hubs])
    constant = "random" not in name
    hub_bound = st.FWD_REL if constant or not split else st.split_row_bound(segments)
    print(f"structured-B forward {name} fwd_fixed={fixed}: worst relative {rel:.3g} on unsplit "
          f"rows (bound {st.FWD_REL:.3g}), {hub:.3g} on the hub rows (bound {hub_bound:.3g})")
    assert rel <= st.FWD_REL
    assert hub <= hub_bound


# ------------------------------------------------------------------------------ C: ranges
# pair chunks (the k = 16 default), lane chunks, and fwd_two_tables alone (k = 16 keeps its pair
# chunks); with fwd_chunk3=2 the plain layouts: the two tables gathered in place, packed records
LAYOUTS = [dict(), dict(fwd_chunk3=3), dict(fwd_chunk3=1), dict(fwd_two_tables=1),
           dict(fwd_chunk3=2, fwd_two_tables=1), dict(fwd_chunk3=2, fwd_two_tables=2)]


def range_plan(gpu, val, layout, fixed, **more):
    p, ix, _ = st.range_graph()
    ptr, idx, dval = graph_on(gpu, p, ix, val)
    opts = dict(layout, fwd_fixed=fixed, fwd_tile_rows=st.RANGE_TILE, **more)
    plan = mk.GraphPlan(ptr, idx, dval, st.RANGE_N, ix.size, st.RANGE_D, st.RANGE_K, options=opts)
    info = plan.info()
    assert info["fwd_tasks"] == st.RANGE_N // st.RANGE_TILE      # tile t = rows [32 t, +32)
    assert info["fwd_fixed"] == (0 if fixed == 2 else 1)
    want = {0: 4, 3: 4, 1: 2, 2: layout.get("fwd_two_tables", 0) - 1}
    assert info["fwd_layout"] == want[layout.get("fwd_chunk3", 0)]
    return plan, dval


def check_range_forward(out, val, data, what):
    """The forward's two bars against the oracle; returns the output."""
    p, ix, _ = st.range_graph()
    _, sel = st.range_tables()
    lo, hi = st.products_normal(p, ix, val, data)
    assert lo >= st.MIN_PRODUCT and hi < 1e30            # precondition: normal f32 products
    ref, mag = oracle.spgemm_forward(p, ix, val, data, sel, st.RANGE_D, with_mag=True)
    out = out.cpu().numpy()
    ok, worst = oracle.close_enough(out, ref, mag, rtol=st.RTOL)
    rel = oracle.worst_relative(out, ref, mag)
    assert ok and rel <= st.FWD_REL, f"{what}: worst err/bound {worst:.3g}, relative {rel:.3g}"
    return out, ref


@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
@pytest.mark.parametrize("case", ["rows", "within", "zeros", "columns"])
def test_range_forward(gpu, case, layout):
    """Edge values whose range grows from 1 to 2^100 between the rows of a tile, inside a row,
    with exact zeros (an all-zero row and tile among them), and a table whose rows span that
    range: fixed point where its bound holds, f64 beyond, the same bars everywhere."""
    _, sel = st.range_tables()
    dsel = to_dev(sel, gpu)
    for e in st.RANGE_E:
        val, data = st.range_values(case, e)
        ddata = to_dev(data, gpu)
        for fixed in (0, 1, 2):
            plan, _ = range_plan(gpu, val, layout, fixed)
            out, ref = check_range_forward(plan.forward(ddata, dsel), val, data,
                                           f"{case} e={e} fwd_fixed={fixed}")
            if case == "within":
                # features 0..15 of a row hold the scaled edge's terms alone: plain relative
                # error on every one of them
                sp = np.abs(out[:, :16].astype(np.float64) / ref[:, :16].astype(np.float64) - 1)
                assert (ref[:, :16] != 0).all() and sp.max() <= st.FWD_REL, (e, fixed, sp.max())
            if case == "zeros":
                rows = np.r_[5, 96:128]
                assert not out[rows].any()


@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
def test_range_forward_mixed_launch(gpu, layout):
    """One launch whose tile 0 is benign and whose tile 1 spans 2^60: with the fixed-point scale
    tile 1's small rows would round to zero, so parity proves that tile 1 fell back; tile 0
    keeps the bits it has in an all-benign launch (same statistics, same scale). Nothing
    observable here tells 'tile 0 fixed, tile 1 f64' from a whole launch in f64: tile 0's slots
    mostly hold a single term, which both paths round alike. By fwd_fix_stats_kernel and
    fwd_fix_scale gexp + ex - en is about 6 on tile 0 and about 66 on tile 1, so the launch is
    mixed; a change to a launch-wide fallback would pass this test."""
    _, sel = st.range_tables()
    val, data = st.range_values("mixed")
    benign, _ = st.range_values("benign")
    ddata, dsel = to_dev(data, gpu), to_dev(sel, gpu)
    for fixed in (0, 1, 2):
        plan, _ = range_plan(gpu, val, layout, fixed)
        out, ref = check_range_forward(plan.forward(ddata, dsel), val, data, f"mixed {fixed}")
        small = out[33:64:2]
        assert small.any() and np.abs(small).max() < 2.0 ** -50
        base, _ = range_plan(gpu, benign, layout, fixed)
        same = base.forward(ddata, dsel).cpu().numpy()
        assert np.array_equal(out[:32].view(np.uint32), same[:32].view(np.uint32))


@pytest.mark.parametrize("layout", LAYOUTS, ids=ids)
@pytest.mark.parametrize("case", ["rows", "within"])
def test_range_forward_follows_value_refresh(gpu, case, layout):
    """refresh_values from the benign values to a range of 2^24, 2^60 and back: the per-task
    decision is recomputed each time."""
    data, sel = st.range_tables()
    ddata, dsel = to_dev(data, gpu), to_dev(sel, gpu)
    for fixed in (0, 1, 2):
        plan, dval = range_plan(gpu, st.range_values("benign")[0], layout, fixed)
        for e in (None, 24, 60, None):
            val = st.range_values("benign" if e is None else case, e or 0)[0]
            dval.copy_(to_dev(val, gpu))
            plan.refresh_values(dval)
            check_range_forward(plan.forward(ddata, dsel), val, data,
                                f"refresh {case} e={e} fwd_fixed={fixed}")


@pytest.mark.parametrize("case", ["rows", "within", "mixed", "zeros"])
def test_range_backward(gpu, case):
    """The backward on the same edge values (gradient magnitudes in [1, 2), so the products
    stay normal), at the 1e-5 bar."""
    p, ix, _ = st.range_graph()
    _, sel = st.range_tables()
    rs = np.random.RandomState(80)
    shape = (st.RANGE_N, st.RANGE_D)
    g = (rs.uniform(1.0, 2.0, shape) * rs.choice([-1.0, 1.0], shape)).astype(np.float32)
    dg, dsel = to_dev(g, gpu), to_dev(sel, gpu)
    for e in st.RANGE_E if case not in ("mixed",) else [60]:
        val, _ = st.range_values(case, e)
        assert np.abs(val[val != 0]).min() * np.abs(g).min() >= st.MIN_PRODUCT
        ref, mag = oracle.sspmm_backward(p, ix, val, g, sel, with_mag=True)
        for opts in (dict(), dict(bwd_algo=3), dict(bwd_features_per_lane=2)):
            ptr, idx, dval = graph_on(gpu, p, ix, val)
            plan = mk.GraphPlan(ptr, idx, dval, st.RANGE_N, ix.size, st.RANGE_D, st.RANGE_K,
                                options=opts)
            got = plan.backward(dg, dsel).cpu().numpy()
            ok, worst = oracle.close_enough(got, ref, mag, rtol=st.RTOL)
            assert ok, f"{case} e={e} {ids(opts)}: worst err/bound {worst:.3g}"


# ------------------------------------------------------------------------------ D: non-finite
@pytest.mark.parametrize("k", [16, 7])
@pytest.mark.parametrize("case", st.NONFINITE_FWD)
def test_nonfinite_forward_vs_oracle(gpu, case, k):
    """A NaN or Inf appears in exactly the outputs whose IEEE sum contains it."""
    c = st.nonfinite_case(k, case)
    for opts in (dict(), dict(fwd_chunk3=3), dict(fwd_fixed=2), dict(fwd_fixed=1)):
        out = plan_for(gpu, c, c.d, k, opts).forward(to_dev(c.od, gpu), to_dev(c.oi, gpu))
        try:
            st.assert_same_nonfinite_and_close(out.cpu().numpy(), c.fwd, c.fwd_mag)
        except AssertionError as exc:
            raise AssertionError(f"{case} k={k} {ids(opts)}: {exc}") from None


@pytest.mark.parametrize("k", [16, 7])
@pytest.mark.parametrize("case", st.NONFINITE_BWD)
def test_nonfinite_backward_vs_oracle(gpu, case, k):
    """k = 7 pads the backward's selector slots, and the padding gathers feature 0: a NaN there
    must reach the slots that select feature 0 and no other."""
    c = st.nonfinite_case(k, case)
    for algo in (1, 3):
        for fpl in (4, 2):
            opts = dict(bwd_algo=algo, bwd_features_per_lane=fpl)
            plan = plan_for(gpu, c, c.d, k, opts)
            assert plan.info()["bwd_algo"] == (algo if k == 16 else 1)
            gs = torch.full((c.n, k), 12345.0, device=gpu)     # every element is written
            plan.backward(to_dev(c.g, gpu), to_dev(c.oi, gpu), gs)
            try:
                st.assert_same_nonfinite_and_close(gs.cpu().numpy(), c.bwd, c.bwd_mag)
            except AssertionError as exc:
                raise AssertionError(f"{case} k={k} {ids(opts)}: {exc}") from None
