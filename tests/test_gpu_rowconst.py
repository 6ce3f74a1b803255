"""GPU: the forward on 4-byte edge words when the edge values are constant per row.

A plan whose forward kernel has the form (tests/rowconst.py, has_rowconst_kernel) keeps the
words {column | row} and one value per row instead of {column | row, value}, sums x with weight
1 and scales each row sum once. Everything here runs against the f64 oracle: bit for bit as
floats where the inputs are exactly summable (integer features, per-row values in {0.5, 1, 2}),
with oracle.close_enough otherwise. plan.info()["fwd_rowconst"] says which stream a plan holds.

k = 8 has no kernel of the form (lane chunks of 3 lanes per edge, no fixed point by default):
its plans must report 0 and stay right; k = 24 runs the lane chunks in the 4-byte form, k = 16
the pair chunks, k = 32 the two tables.
"""
import numpy as np
import pytest
import torch

import maxk_kernels as mk
import rowconst as rc
import structured as st
from oracle import oracle
from test_gpu_parity import assert_close, graph_on, to_dev
from test_gpu_structured import assert_equal_floats

pytestmark = pytest.mark.gpu

KS = (8, 16, 24, 32)
LAYOUT = {8: 2, 16: 4, 24: 2, 32: 0}


def plan_for(gpu, c, opts=None):
    ptr, idx, val = graph_on(gpu, c.p, c.ix, c.v)
    return mk.GraphPlan(ptr, idx, val, c.n, c.ix.size, rc.D, c.k, num_cols=c.od.shape[0],
                        options=opts or {})


def tables(gpu, c):
    return to_dev(c.od, gpu), to_dev(c.oi, gpu)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("gname", list(rc.GRAPHS))
def test_exact_forward_and_accumulate(gpu, gname, k):
    """Whole tiles, a partial one, an edgeless one, rows of 0 and 1 edges (tiles); a row split
    into segments (heavy). The 4-byte plan, the forced 8-byte plan and a continuing launch all
    equal the oracle as floats."""
    c = rc.exact_case(gname, k)
    assert st.exactly_summable(c.mag)
    plan = plan_for(gpu, c)
    info = plan.info()
    assert info["fwd_rowconst"] == int(rc.has_rowconst_kernel(k)) == (0 if k == 8 else 1)
    assert info["fwd_layout"] == LAYOUT[k]
    if gname == "tiles":
        assert info["fwd_tasks"] == 5 and info["fwd_split_rows"] == 0
    else:
        assert info["fwd_split_rows"] == 1
    sd, si = tables(gpu, c)
    out = plan.forward(sd, si)
    assert_equal_floats(out, c.ref, f"forward {gname} k={k}")
    assert (out[np.flatnonzero(np.diff(c.p) == 0)] == 0).all()      # edgeless rows
    wide = plan_for(gpu, c, dict(fwd_rowconst=2))
    assert wide.info()["fwd_rowconst"] == 0
    assert_equal_floats(wide.forward(sd, si), c.ref, f"8-byte forward {gname} k={k}")
    # a continuing launch: the prior row is added after the scaling (integers: still exact)
    pre = st.int_features(c.n, rc.D, seed=7)
    acc = plan.forward(sd, si, out=to_dev(pre, gpu).clone(), accumulate=True)
    assert st.exactly_summable(c.mag + np.abs(pre))
    assert_equal_floats(acc, c.ref.astype(np.float64) + pre, f"accumulate {gname} k={k}")


@pytest.mark.parametrize("gname", list(rc.GRAPHS))
def test_exact_forward_records(gpu, gname):
    """The records entry point at k = 16 (pair-chunk records written by the top-k) shares the
    kernel: 4-byte words, equal to the oracle as floats, accumulate included."""
    c = rc.exact_case(gname, 16)
    plan = plan_for(gpu, c)
    assert plan.info()["fwd_rowconst"] == 1
    rec, layout = plan.new_records()
    assert layout == 4
    stats = torch.empty(2, dtype=torch.int32, device=gpu)
    sd, si = mk.maxk_forward(to_dev(c.x, gpu), 16, return_index=True, records=(rec, layout),
                             stats=stats)
    assert np.array_equal(sd.cpu().numpy(), c.od) and np.array_equal(si.cpu().numpy(), c.oi)
    out = plan.forward_records(rec, layout, stats=stats.view(1, 2))
    assert_equal_floats(out, c.ref, f"forward_records {gname}")
    pre = st.int_features(c.n, rc.D, seed=8)
    acc = plan.forward_records(rec, layout, out=to_dev(pre, gpu).clone(), accumulate=True,
                               stats=stats.view(1, 2))
    assert_equal_floats(acc, c.ref.astype(np.float64) + pre, f"forward_records accumulate {gname}")


@pytest.mark.parametrize("k", (16, 24, 32))
def test_duplicate_selectors(gpu, k):
    """Repeated selectors inside a table row are summed (the statistics then bound a slot by the
    row's sum |x|)."""
    c = rc.exact_case("tiles", k, dup=True)
    assert st.exactly_summable(c.mag)
    plan = plan_for(gpu, c)
    assert plan.info()["fwd_rowconst"] == 1
    assert_equal_floats(plan.forward(*tables(gpu, c)), c.ref, f"duplicate selectors k={k}")


def test_fixed_and_f64_tasks_in_one_launch(gpu):
    """structured's wide-range tables with row-constant values: the 8-edge tiles run fixed
    point, the 128-edge tile f64 (rc.fixed_tasks replays the per-task rule for unit weights),
    each within the fp32-accumulator bar."""
    c = rc.range_case()
    assert rc.fixed_tasks(c.p, c.od) == [True, False, True]
    plan = plan_for(gpu, c)
    info = plan.info()
    assert info["fwd_rowconst"] == 1 and info["fwd_fixed"] == 1 and info["fwd_tasks"] == 3
    out = plan.forward(*tables(gpu, c))
    assert_close(out, c.ref, c.mag)
    # bitwise reproducible run to run (integer sums; one f64 add order per f64 slot is not
    # promised, so only the fixed-point tiles are compared)
    again = plan.forward(*tables(gpu, c))
    assert torch.equal(out[:32], again[:32]) and torch.equal(out[64:], again[64:])


@pytest.mark.parametrize("k", (16, 32))
def test_one_changed_edge_value_falls_back(gpu, k):
    """The same graph with a single edge value changed in one row takes the 8-byte words, and
    computes bit for bit what the forced 8-byte plan does."""
    c = rc.exact_case("tiles", k, break_row=50)
    assert rc.rowconst_rule(c.p, c.v) == 0
    plan = plan_for(gpu, c)
    assert plan.info()["fwd_rowconst"] == 0
    wide = plan_for(gpu, c, dict(fwd_rowconst=2))
    sd, si = tables(gpu, c)
    out, ref8 = plan.forward(sd, si), wide.forward(sd, si)
    assert torch.equal(out.view(torch.int32), ref8.view(torch.int32))
    assert plan.info()["device_bytes"] == wide.info()["device_bytes"]
    assert_equal_floats(out, c.ref, f"fallback k={k}")


@pytest.mark.parametrize("k", (16, 32))
def test_refresh_switches_the_stream_both_ways(gpu, k):
    """constant -> not constant -> constant (other values): fwd_rowconst 1, 0, 1, the oracle at
    every step, and the plan's reported memory smaller by the value half of the words less the
    row values: 4 (E + 1) - 4 N bytes (the stream carries one word past the end)."""
    steps = [rc.exact_case("tiles", k), rc.exact_case("tiles", k, break_row=50),
             rc.exact_case("tiles", k, values_seed=2)]
    c = steps[0]
    e, n = c.ix.size, c.n
    ptr, idx, val = graph_on(gpu, c.p, c.ix, c.v)
    plan = mk.GraphPlan(ptr, idx, val, n, e, rc.D, k, num_cols=rc.NCOLS)
    sd, si = tables(gpu, c)
    seen, sizes = [], []
    for i, s in enumerate(steps):
        if i:
            val.copy_(to_dev(s.v, gpu))
            plan.refresh_values(val)
        info = plan.info()
        seen.append(info["fwd_rowconst"])
        sizes.append(info["device_bytes"])
        assert info["fwd_rowconst"] == rc.rowconst_rule(s.p, s.v)
        assert_equal_floats(plan.forward(sd, si), s.ref, f"refresh step {i} k={k}")
    assert seen == [1, 0, 1]
    assert sizes[0] == sizes[2] and sizes[1] - sizes[0] == 4 * (e + 1) - 4 * n
    wide = mk.GraphPlan(ptr, idx, val, n, e, rc.D, k, num_cols=rc.NCOLS,
                        options=dict(fwd_rowconst=2))
    assert wide.info()["device_bytes"] == sizes[1] and wide.info()["fwd_rowconst"] == 0
    # a forced 8-byte plan stays so through a refresh with row-constant values
    wide.refresh_values(val)
    assert wide.info()["fwd_rowconst"] == 0
    assert_equal_floats(wide.forward(sd, si), steps[2].ref, f"8-byte refresh k={k}")


@pytest.mark.parametrize("kind", ("val_nan", "val_inf", "table"))
@pytest.mark.parametrize("k", (16, 32))
def test_nonfinite(gpu, k, kind):
    """A row whose constant is NaN or +-Inf keeps the plan on the 8-byte words; non-finite table
    entries under finite row values run the 4-byte form. Either way NaN, +Inf and -Inf stand
    exactly where the oracle's IEEE sums have them."""
    c = rc.nonfinite_case(k, kind)
    plan = plan_for(gpu, c)
    assert plan.info()["fwd_rowconst"] == rc.rowconst_rule(c.p, c.v) == (1 if kind == "table" else 0)
    out = plan.forward(*tables(gpu, c)).cpu().numpy()
    st.assert_same_nonfinite_and_close(out, c.ref, c.mag)
    # refreshing a finite row-constant plan to the non-finite constants falls back too
    if kind != "table":
        fin = rc.exact_case("tiles", k)
        ptr, idx, val = graph_on(gpu, fin.p, fin.ix, fin.v)
        p2 = mk.GraphPlan(ptr, idx, val, c.n, c.ix.size, rc.D, k, num_cols=rc.NCOLS)
        assert p2.info()["fwd_rowconst"] == 1
        val.copy_(to_dev(c.v, gpu))
        p2.refresh_values(val)
        assert p2.info()["fwd_rowconst"] == 0
        out2 = p2.forward(*tables(gpu, c)).cpu().numpy()
        st.assert_same_nonfinite_and_close(out2, c.ref, c.mag)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("gname", list(rc.GRAPHS))
def test_rule_agrees_with_the_plan(gpu, gname, k):
    """The numpy rule and the plan's report on the same graphs: constant, one value changed,
    unit weights (val of ones), a zero and a NaN constant."""
    p, ix = rc.GRAPHS[gname]()
    n = p.size - 1
    base = rc.exact_case(gname, k).v
    row = int(np.flatnonzero(np.diff(p) >= 2)[0])
    cases = {"constant": base, "ones": np.ones_like(base)}
    for name, x in (("changed", 4.0), ("zero", 0.0), ("nan", np.nan)):
        v = base.copy()
        if name == "changed":
            v[p[row] + 1] = x
        else:
            v[p[row]:p[row + 1]] = x
        cases[name] = v
    for name, v in cases.items():
        ptr, idx, val = graph_on(gpu, p, ix, v)
        plan = mk.GraphPlan(ptr, idx, val, n, ix.size, rc.D, k, num_cols=rc.NCOLS)
        want = rc.rowconst_rule(p, v) if rc.has_rowconst_kernel(k) else 0
        assert plan.info()["fwd_rowconst"] == want, (name, k)
    assert [rc.rowconst_rule(p, v) for v in cases.values()] == [1, 1, 0, 0, 0]


def test_capture_and_replay(gpu):
    """One capture of the 4-byte forward, replayed on other table contents, against eager."""
    c = rc.exact_case("heavy", 16)
    plan = plan_for(gpu, c)
    assert plan.info()["fwd_rowconst"] == 1
    sd, si = tables(gpu, c)
    other = rc.exact_case("heavy", 16, dup=True)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        out = torch.empty((c.n, rc.D), device=gpu)
        plan.forward(sd, si, out=out)                      # warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            plan.forward(sd, si, out=out)
        for case in (other, c):
            sd.copy_(to_dev(case.od, gpu))
            si.copy_(to_dev(case.oi, gpu))
            out.fill_(float("nan"))
            g.replay()
            side.synchronize()
            got = out.clone()
            eager = plan.forward(sd, si)
            side.synchronize()
            assert torch.equal(got.view(torch.int32), eager.view(torch.int32))
            assert_equal_floats(got, case.ref, "replay")
    torch.cuda.current_stream(gpu).wait_stream(side)
