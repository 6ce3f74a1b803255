"""CPU: what tests/autograd_drivers.py builds for tests/test_gpu_autograd_drivers.py.

* the surface table covers every Function class of maxk_kernels.autograd and every operator of
  maxk_kernels.torch_ops that has a derivative, and the not-applicable table is within its cap;
* every sum a driver forms stays exact: one gradient doubled (drivers 1, 4), sums of two (2, 4),
  three (4: one table, one x) and so at most four gradients, on the graph's own values, on values
  doubled in place (6b) and, for the weighted surfaces, on values times weights from
  {0.5, 1, 2} (quantum 0.25 instead of 0.5);
* the cases are the sweep's own (exact mode) and built as structured.exact_case builds them
  (ref_compat), and the variants really differ, so a driver that mixed two calls up, or computed
  with edited values, could not pass;
* `first_order_only` and the edge-value version check, on a Function that needs no GPU.
"""
import types

import numpy as np
import pytest
import torch

import autograd_drivers as ad
import sweep
from maxk_kernels import autograd
from structured import EXACT_LIMIT, exactly_summable

CONFIGS = [(g, d, k) for g in ad.GRAPHS for d, k in ad.DK]
EXACT = [S for S in ad.SURFACES if S.exact]


def quantum(S):
    return 0.25 if len(S.inputs) == 2 else 0.5


# ------------------------------------------------------------------ the tables
def test_every_function_and_operator_has_a_surface():
    covered = {c for S in ad.SURFACES for c in S.covers}
    assert set(ad.autograd_functions()) <= covered, set(ad.autograd_functions()) - covered
    assert set(ad.operators_with_derivative()) <= covered
    assert covered <= set(ad.autograd_functions()) | set(ad.operators_with_derivative())
    assert len(ad.autograd_functions()) == 8 and len(ad.operators_with_derivative()) == 5
    assert len({S.name for S in ad.SURFACES}) == len(ad.SURFACES)


def test_not_applicable_table_is_within_its_cap():
    names = ad.autograd_functions() + ad.operators_with_derivative()
    pairs = {(n, drv) for n in names for drv in ad.DRIVERS}
    assert set(ad.NOT_APPLICABLE) <= pairs
    assert all(isinstance(r, str) and r.strip() for r in ad.NOT_APPLICABLE.values())
    assert len(ad.NOT_APPLICABLE) <= ad.NOT_APPLICABLE_CAP * len(pairs)
    assert ad.NOT_APPLICABLE_CAP == 0.15 and len(ad.DRIVERS) == 12


def test_configurations_are_the_issue_s():
    assert ad.DK == [(256, 16), (64, 8), (100, 10)] and ad.PS == (0.0, 0.5)
    assert ad.MODES == ("exact", "ref_compat") and ad.N == 600
    for S in ad.SURFACES:
        envs = S.envs("sparse", 64, 8)
        assert len(envs) == (2 if S.takes_drop else 1) * (2 if S.takes_mode else 1)


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("gname,d,k", CONFIGS)
def test_cases_are_the_sweep_s(gname, d, k):
    """Exact mode, variant 0: sweep.case's own tables, output and x.grad."""
    S = ad.BY_NAME["maxk_aggregate"]
    for p in ad.PS:
        c, mine = sweep.case(gname, d, k, p), ad.case(gname, d, k, p)
        assert np.array_equal(mine.x, c.x) and np.array_equal(mine.oi, c.oi)
        assert np.array_equal(mine.od, c.od) and mine.filled.all()
        E = ad.env(gname, d, k, p)
        assert np.array_equal(S.np_gouts(E)[0], c.g)
        assert np.array_equal(S.ref_outs(E)[0], c.fwd)
        assert np.array_equal(S.ref_grads(E, (c.g,))["x"], c.gx)
        assert np.array_equal(S.ref_grads(E, (c.g,), mag=True)["x"], c.gx_mag)


@pytest.mark.parametrize("gname,d,k", CONFIGS)
def test_ref_compat_rows_are_built_as_exact_case_builds_them(gname, d, k):
    """Filled slots first, padding (0.0f, selector 0) behind them; where no selected value is
    zero, `filled` is structured.exact_case's `od0 != 0`."""
    padded = 0
    for xvar in range(3):
        c = ad.case(gname, d, k, 0.0, "ref_compat", xvar)
        assert (c.od0[~c.filled] == 0).all() and (c.oi[~c.filled] == 0).all()
        assert (c.count >= 0).all() and (c.count <= k).all()
        nonzero = c.od0 != 0
        assert not (nonzero & ~c.filled).any()
        if xvar == 0:
            assert np.array_equal(nonzero, c.filled)
        padded += int((~c.filled).sum())
    # the integer rows of D = 256 always fill 16 slots; the two narrower cases have padded rows
    assert (padded > 0) == (d < 256)


def test_weights_and_values_are_dyadic():
    for gname in ad.GRAPHS:
        assert set(np.unique(sweep.graph(gname)[2])) <= {0.5, 1.0, 2.0}
        for wvar in range(3):
            w = ad.weights(gname, wvar)
            assert w.shape == (sweep.edges(gname),) and set(np.unique(w)) == {0.5, 1.0, 2.0}
        assert not np.array_equal(ad.weights(gname, 0), ad.weights(gname, 1))


# ------------------------------------------------------------------ exactness of every sum
@pytest.mark.parametrize("gname,d,k", CONFIGS)
def test_every_sum_the_drivers_form_is_exact(gname, d, k):
    """Four times the largest sum of |terms| of any single gradient or output stays within the
    exact range, for every surface, configuration, data variant, gradient variant and value
    scale the drivers use; and each restated gradient is itself an f32 number."""
    for S in EXACT:
        for E in S.envs(gname, d, k):
            for var in range(3):
                for vscale in (1.0, 2.0) if S.uses_graph_val and var == 1 else (1.0,):
                    gs = S.np_gouts(E, var)
                    mag = S.ref_grads(E, gs, xvar=var, wvar=var, vscale=vscale, mag=True)
                    ref = S.ref_grads(E, gs, xvar=var, wvar=var, vscale=vscale)
                    for n in S.inputs:
                        assert ad.exact_sum_ok(mag[n], 4, quantum(S)), (S, vars(E), var, n)
                        assert np.array_equal(ref[n], ref[n].astype(np.float32))
                        assert (np.abs(ref[n]) <= mag[n]).all()
                        assert (ref[n] / quantum(S) == np.round(ref[n] / quantum(S))).all()
            ones = tuple(np.ones_like(g) for g in S.np_gouts(E))       # driver 10's y.sum()
            for n, m in S.ref_grads(E, ones, mag=True).items():
                assert ad.exact_sum_ok(m, 4, quantum(S))


@pytest.mark.parametrize("gname,d,k", CONFIGS)
def test_fan_out_of_one_x_through_two_k_is_exact(gname, d, k):
    for p in ad.PS:
        for mode in ad.MODES:
            c = ad.case(gname, d, k, p, mode)
            c2 = ad.case(gname, d, k // 2, p, mode, 0, ad.SEED, 1.0, k)
            assert np.array_equal(c2.x, c.x) and c2.oi.shape == (ad.N, k // 2)
            total = (ad.x_grad(c, ad.grad_nd(d, k, 0), mag=True) +
                     ad.x_grad(c, ad.grad_nd(d, k, 1), mag=True) +
                     ad.x_grad(c2, ad.grad_nd(d, k, 2), mag=True) +
                     ad.x_grad(c, g_slots=ad.grad_nk(k, 0), mag=True))
            assert exactly_summable(total)


def test_exact_sum_ok_is_the_suite_s_limit():
    assert ad.exact_sum_ok(np.array([EXACT_LIMIT]), 1, 0.5)
    assert not ad.exact_sum_ok(np.array([EXACT_LIMIT + 1]), 1, 0.5)
    assert ad.exact_sum_ok(np.array([EXACT_LIMIT / 8]), 4, 0.25)
    assert not ad.exact_sum_ok(np.array([EXACT_LIMIT / 8 + 1]), 4, 0.25)
    assert not ad.exact_sum_ok(np.array([np.inf]), 1, 0.5)
    # the largest sums of |terms| of the plain cases: far below the limit of 4,194,304
    worst = {"fwd": 0.0, "gx": 0.0}
    for gname, d, k in CONFIGS:
        for p in ad.PS:
            c = sweep.case(gname, d, k, p)
            worst["fwd"] = max(worst["fwd"], float(c.fwd_mag.max()))
            worst["gx"] = max(worst["gx"], float(c.gx_mag.max()))
    assert worst["fwd"] <= 9604.0 and worst["gx"] <= 2315.0, worst


# ------------------------------------------------------------------ the variants differ
@pytest.mark.parametrize("gname,d,k", CONFIGS[::3])
def test_variants_and_edited_values_give_other_gradients(gname, d, k):
    for S in EXACT:
        E = S.envs(gname, d, k)[-1]
        g0 = S.np_gouts(E, 0)
        base = S.ref_grads(E, g0)
        for n in S.inputs:
            other = S.ref_grads(E, S.np_gouts(E, 1))
            assert not np.array_equal(base[n], other[n]), (S, n, "gradient variants")
        for var in (1, 2):
            moved = S.ref_grads(E, g0, xvar=var, wvar=var)
            outs = zip(S.ref_outs(E), S.ref_outs(E, xvar=var, wvar=var))
            # (the plain dense aggregation is linear: its gradient does not depend on x)
            assert (any(not np.array_equal(base[n], moved[n]) for n in S.inputs) or
                    S.name == "dense_aggregate"), (S, var)
            assert any(not np.array_equal(a, b) for a, b in outs), (S, var)
        if S.uses_graph_val:
            edited = S.ref_grads(E, g0, vscale=2.0)
            n = S.inputs[0]
            assert not np.array_equal(base[n], edited[n]), (S, "graph.val doubled")


# ------------------------------------------------------------------ the product's two guards
class _Opaque(torch.autograd.Function):
    """A backward autograd cannot see through, as a ctypes launch into torch.empty is."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(w)
        return (x * w).detach().clone()

    @staticmethod
    @autograd.first_order_only
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        out = torch.empty_like(g)
        out.copy_(g * w)
        return out, None


@pytest.mark.parametrize("power", [1, 2])
def test_first_order_only_raises_on_a_second_differentiation(power):
    """A constant incoming gradient (power 1: y.sum()) and one that requires grad (power 2):
    the first-order value is right, and the penalty's backward raises instead of dropping it."""
    x = torch.arange(5.0, requires_grad=True)
    w = torch.arange(5.0) + 1
    y = _Opaque.apply(x, w)
    loss = (y ** power).sum()
    (gx,) = torch.autograd.grad(loss, x, create_graph=True)
    assert torch.equal(gx.detach(), power * y.detach() ** (power - 1) * w) and gx.requires_grad
    with pytest.raises(RuntimeError, match="differentiate twice"):
        (loss + gx.pow(2).sum()).backward()
    x.grad = None
    (_Opaque.apply(x, w) ** power).sum().backward()        # plain use is unchanged
    assert torch.equal(x.grad, gx.detach())


def test_inference_tensors_have_no_version_to_read():
    """ops._version: the counter of a normal tensor, 0 for an inference tensor (reading its
    _version raises), -1 for no tensor; what the plans and the value check compare."""
    from maxk_kernels import ops
    t = torch.ones(3)
    assert ops._version(t) == t._version == 0 and ops._version(None) == -1
    t.add_(1.0)
    assert ops._version(t) == 1
    with torch.inference_mode():
        inf = torch.ones(3)
    with pytest.raises(RuntimeError, match="version counter"):
        inf._version
    assert ops._version(inf) == 0


def test_edge_value_version_check():
    val = torch.ones(4)
    ctx = types.SimpleNamespace()
    autograd._save_values_version(ctx, val)
    autograd._check_values_version(ctx)
    val[1:].mul_(2.0)                                       # through a view
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        autograd._check_values_version(ctx)
