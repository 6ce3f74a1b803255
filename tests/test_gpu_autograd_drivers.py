"""GPU: every autograd surface under every way a training script drives autograd.

Every other test builds a fresh graph, calls .backward() once and differentiates every input.
Here the surfaces of tests/autograd_drivers.py (the public functions of maxk_kernels.autograd,
with and without edge_weight=, the edge softmax, and every torch.ops.maxk operator that has a
derivative) run under twelve drivers:

 1 twice through one graph (retain_graph)      7 create_graph=True (values; a second
 2 accumulation into .grad over two steps        differentiation must raise, never drop a term)
 3 partial gradients, with launch counts       8 torch.utils.checkpoint, both flavours
 4 fan-out of one tensor into several calls    9 no_grad / inference_mode
 5 interleaved lifetimes on one plan          10 incoming gradient layouts
 6 in-place edits between forward and         11 input layouts (views of a larger leaf)
   backward                                   12 forward on a side stream, backward outside

and the four layers under drivers 2, 3, 7 and 8. The last test is the closure: every Function
class of maxk_kernels.autograd and every operator with a derivative of maxk_kernels.torch_ops ran
under every driver (or is listed in autograd_drivers.NOT_APPLICABLE with a reason).

Inputs are the exactly summable cases of tests/sweep.py (tests/test_autograd_driver_inputs.py
holds their preconditions), so two routes to one gradient are compared with np.array_equal
against the f64 restatement. Two kinds of case are not bit-reproducible and are compared
otherwise, with the bars the suite already has:

* edge_softmax has no exact inputs. It is deterministic, so the drivers compare with the plain
  `ops` calls bit for bit, and test_edge_softmax_restatement_within_its_bounds holds those to
  the float64 bounds of tests/test_gpu_edge_softmax.py.
* the layers multiply by real-valued weights, so the SSpMM's float atomics add in an order that
  changes the last bits from run to run: layer gradients, checkpointed or not, are compared with
  the f64 dense restatements under the norm-wise `close` of tests/test_layers.py (1e-5 / 2e-5),
  not with each other.
"""
import collections
import gc
import itertools
import weakref

import numpy as np
import pytest
import torch
from torch.utils.checkpoint import checkpoint

import autograd_drivers as ad
import maxk_kernels as mk
from autograd_drivers import C, SURFACES, env, f32, to_dev
from maxk_kernels import graphs, ops
from test_dropout_capi import drop_scale, keep_mask
from test_edge_softmax_capi import backward_bound, forward_bound, softmax_rows64
from test_layers import close, dense_adj

pytestmark = pytest.mark.gpu

CONFIGS = [(g, d, k) for g in ad.GRAPHS for d, k in ad.DK]
config = pytest.mark.parametrize("gname,d,k", CONFIGS)
RAN = set()                                   # (covered Function or operator, driver)
COUNTS = collections.Counter()                # driver -> (surface, configuration) cases run
STARTED = set()                               # (driver, configuration) blocks that began
INPLACE = "inplace|in-place"


@pytest.fixture(autouse=True)
def _device(gpu):
    ad.DEVICE = gpu


def cases(driver, gname, d, k, surfaces=SURFACES):
    """Every (surface, configuration) of one block, marked as run under `driver`."""
    STARTED.add((driver, gname, d, k))
    for S in surfaces:
        for E in S.envs(gname, d, k):
            yield S, E
            for c in S.covers:
                RAN.add((c, driver))
            COUNTS[driver] += 1


def leaves(S, E, dev, req=None, xvar=0, wvar=0):
    """Device tensors of the surface's inputs; those named in `req` (default: every
    differentiable input) are leaves that require grad."""
    t = {}
    for n, a in S.np_inputs(E, xvar, wvar).items():
        t[n] = to_dev(a, dev)
        if n in S.inputs and (req is None or n in req):
            t[n].requires_grad_(True)
    return t


def gouts(S, E, dev, gvar=0):
    return tuple(to_dev(g, dev) for g in S.np_gouts(E, gvar))


def backward(outs, gs, **kw):
    pairs = [(o, g) for o, g in zip(outs, gs) if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs], **kw)


def refs(S, E, gvar=0, **kw):
    return {n: f32(a) for n, a in S.ref_grads(E, S.np_gouts(E, gvar), **kw).items()}


def same(got, ref, what):
    """np.array_equal against the restatement, with the first difference in the message; a
    gradient autograd did not produce (None) stands for zeros."""
    ref = np.asarray(ref).astype(np.float32)
    if got is None:
        assert not ref.any(), f"{what}: no gradient, but the restatement is not zero"
        return
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = got != ref
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at "
                             f"{at}: got {got[bad][:4]}, expected {ref[bad][:4]}")


def check_grads(S, E, t, R, what, names=None):
    for n in names or S.inputs:
        same(t[n].grad, R[n], f"{S} {vars(E)} {what}: d/d{n}")


def check_outs(S, E, outs, what, **kw):
    for i, (o, r) in enumerate(zip(outs, S.ref_outs(E, **kw))):
        same(o, r, f"{S} {vars(E)} {what}: output {i}")


def subsets(names):
    return [c for r in range(1, len(names) + 1) for c in itertools.combinations(names, r)]


@pytest.fixture
def launches(monkeypatch):
    """Counts the library calls behind each kind of gradient, by wrapping them as
    test_gpu_self.py and test_gpu_edge_softmax.py do."""
    n = collections.Counter()

    def wrap(owner, name, key):
        real = getattr(owner, name)

        def counted(*a, **k):
            n[key] += 1
            return real(*a, **k)
        monkeypatch.setattr(owner, name, counted)

    wrap(ops.GraphPlan, "backward", "sspmm")
    wrap(ops, "spgemm_edge_grad", "sddmm")
    wrap(ops, "maxk_backward", "scatter")
    wrap(ops, "dense_spmm", "dense_spmm")
    wrap(ops, "edge_softmax_backward", "softmax_backward")
    return n


# ------------------------------------------------------------------ the softmax restatement
@pytest.mark.parametrize("gname", ad.GRAPHS)
def test_edge_softmax_restatement_within_its_bounds(gpu, gname):
    """What the drivers compare the edge softmax with (the plain ops calls) is within
    forward_bound of the float64 softmax, and the plain autograd gradient within backward_bound
    plus the error carried from the forward (the derivation is in
    test_gpu_edge_softmax.test_autograd_gradient_within_bound)."""
    S, E = ad.BY_NAME["edge_softmax"], env(gname, 64, 8)
    ptr, x, w = ad.sweep.graph(gname)[0], ad.logits(gname, 0), ad.grad_edges(gname, 0)
    y64 = softmax_rows64(ptr, x)
    yh = S.ref_outs(E)[0]
    assert (np.abs(yh.astype(np.float64) - y64) <= forward_bound(ptr, x)).all()
    t = leaves(S, E, gpu)
    outs = S.fwd(E, ad.shared_graph(gpu, gname), t)
    same(outs[0], yh, "autograd forward")
    backward(outs, gouts(S, E, gpu))
    same(t["logits"].grad, S.ref_grads(E, (w,))["logits"], "autograd gradient")
    w64 = w.astype(np.float64)
    rows = ad.edge_rows(gname)
    s_abs, tsum, eps = np.zeros(ad.N), np.zeros(ad.N), np.zeros(ad.N)
    np.add.at(s_abs, rows, np.abs(y64 * w64))
    np.add.at(tsum, rows, y64 * w64)
    np.maximum.at(eps, rows, forward_bound(ptr, x) / y64)
    eps = eps[rows]
    carried = eps * (1 + eps) * y64 * (np.abs(w64) + 2 * s_abs[rows])
    err = np.abs(t["logits"].grad.cpu().numpy().astype(np.float64) - y64 * (w64 - tsum[rows]))
    assert (err <= backward_bound(ptr, yh, w) + carried).all()


# ------------------------------------------------------------------ 1: twice through one graph
@config
def test_driver01_twice_through_one_graph(gpu, gname, d, k):
    """backward(retain_graph=True), backward() again, then autograd.grad through the same graph:
    the first gradient is the restatement, .grad after two passes is twice it, and the third
    pass returns the first one's bits."""
    graph = ad.shared_graph(gpu, gname)
    for S, E in cases(1, gname, d, k):
        t, gs, R = leaves(S, E, gpu), gouts(S, E, gpu), refs(S, E)
        outs = S.fwd(E, graph, t)
        check_outs(S, E, outs, "forward")
        backward(outs, gs, retain_graph=True)
        first = {n: t[n].grad.clone() for n in S.inputs}
        check_grads(S, E, t, R, "first pass")
        backward(outs, gs, retain_graph=True)
        check_grads(S, E, t, {n: R[n] + R[n] for n in R}, "two passes accumulated")
        pairs = [(o, g) for o, g in zip(outs, gs)]
        third = torch.autograd.grad([o for o, _ in pairs], [t[n] for n in S.inputs],
                                    [g for _, g in pairs])
        for n, g3 in zip(S.inputs, third):
            assert torch.equal(g3, first[n]), f"{S} {vars(E)}: third pass d/d{n} differs"


# ------------------------------------------------------------------ 2: accumulation
@config
def test_driver02_accumulation_over_two_steps(gpu, gname, d, k):
    """Two forward/backward steps with different incoming gradients and no zero_grad: .grad is
    the f32 sum of the two restatements."""
    graph = ad.shared_graph(gpu, gname)
    for S, E in cases(2, gname, d, k):
        t = leaves(S, E, gpu)
        for gvar in (0, 1):
            backward(S.fwd(E, graph, t), gouts(S, E, gpu, gvar))
        R0, R1 = refs(S, E, 0), refs(S, E, 1)
        check_grads(S, E, t, {n: R0[n] + R1[n] for n in R0}, "two steps")


# ------------------------------------------------------------------ 3: partial gradients
def _expect_no_launch(S, req, used, n, what):
    """No SSpMM, scatter or transposed SpMM when the features' gradient is not asked for, no
    SDDMM when the edge values' is not, and neither when the aggregated output is unused."""
    feats = S.inputs[0] in req
    vals = len(S.inputs) == 2 and S.inputs[1] in req
    agg_used = used[-1]
    if not (feats and agg_used):
        assert n["sspmm"] == 0, (what, dict(n))
    if not feats:
        assert n["scatter"] == 0 and n["dense_spmm"] == 0 and n["softmax_backward"] == 0, \
            (what, dict(n))
    if not (vals and agg_used):
        assert n["sddmm"] == 0, (what, dict(n))


@config
def test_driver03_partial_gradients(gpu, gname, d, k, launches):
    """autograd.grad for every non-empty subset of the inputs (the others constant) and of the
    outputs: each result is the matching piece of the full restatement, and no kernel runs for
    a gradient that is not asked for. Then with every input a leaf and backward(inputs=subset):
    the inputs left out keep .grad None."""
    graph = ad.shared_graph(gpu, gname)
    for S, E in cases(3, gname, d, k):
        n_out = len(S.np_gouts(E))
        for req in subsets(S.inputs):
            for used in itertools.product((True, False), repeat=n_out):
                if not any(used):
                    continue
                what = f"{S} {vars(E)} inputs {req} outputs {used}"
                t, gs = leaves(S, E, gpu, req), gouts(S, E, gpu)
                outs = S.fwd(E, graph, t)
                pairs = [(o, g) for o, g, u in zip(outs, gs, used) if u]
                launches.clear()
                got = torch.autograd.grad([o for o, _ in pairs], [t[n] for n in req],
                                          [g for _, g in pairs], allow_unused=True)
                _expect_no_launch(S, req, used, launches, what)
                R = S.ref_grads(E, tuple(g if u else None
                                         for g, u in zip(S.np_gouts(E), used)))
                for n, g in zip(req, got):
                    same(g, R[n], f"{what}: d/d{n}")
                for n in S.inputs:
                    assert t[n].grad is None
        R = refs(S, E)
        for req in subsets(S.inputs):
            t = leaves(S, E, gpu)
            backward(S.fwd(E, graph, t), gouts(S, E, gpu), inputs=[t[n] for n in req])
            check_grads(S, E, t, R, f"backward(inputs={req})", req)
            assert all(t[n].grad is None for n in S.inputs if n not in req)


# ------------------------------------------------------------------ 4: fan-out
@config
def test_driver04_fan_out(gpu, gname, d, k):
    """One set of leaves feeds every surface twice, with different incoming gradients, and one
    backward runs through both: the gradient is the sum of the parts."""
    graph = ad.shared_graph(gpu, gname)
    for S, E in cases(4, gname, d, k):
        t = leaves(S, E, gpu)
        outs = S.fwd(E, graph, t) + S.fwd(E, graph, t)
        backward(outs, gouts(S, E, gpu, 0) + gouts(S, E, gpu, 1))
        R0, R1 = refs(S, E, 0), refs(S, E, 1)
        check_grads(S, E, t, {n: R0[n] + R1[n] for n in R0}, "fed twice")


@config
@pytest.mark.parametrize("p", ad.PS)
@pytest.mark.parametrize("mode", ad.MODES)
def test_driver04_fan_out_of_one_table_and_of_one_x(gpu, gname, d, k, p, mode):
    """sp_data of one maxk feeds two spgemm calls and a direct term; one x feeds maxk_aggregate
    twice with the same k (one shared plan) and once with another k."""
    graph = ad.shared_graph(gpu, gname)
    E = env(gname, d, k, p, mode)
    c = C(E)
    g0, g1, gk = ad.grad_nd(d, k, 0), ad.grad_nd(d, k, 1), ad.grad_nk(k, 0)
    x = to_dev(c.x, gpu).requires_grad_(True)
    sp, si = mk.maxk(x, k, mode, dropout_p=p, seed=ad.SEED)
    y0, y1 = mk.spgemm(sp, si, graph, d), mk.spgemm(sp, si, graph, d)
    torch.autograd.backward([y0, y1, (sp * to_dev(gk, gpu)).sum()],
                            [to_dev(g0, gpu), to_dev(g1, gpu), None])
    same(x.grad, ad.x_grad(c, g0) + ad.x_grad(c, g1) + ad.x_grad(c, g_slots=gk),
         f"{vars(E)}: one table, two spgemm and a direct term")

    k2 = k // 2
    E2 = env(gname, d, k2, p, mode)
    g2 = ad.grad_nd(d, k, 2)
    x = to_dev(c.x, gpu).requires_grad_(True)
    kw = dict(dropout_p=p, seed=ad.SEED)
    ys = [mk.maxk_aggregate(x, graph, k, mode, **kw), mk.maxk_aggregate(x, graph, k, mode, **kw),
          mk.maxk_aggregate(x, graph, k2, mode, **kw)]
    assert graph.plan(d, k) is graph.plan(d, k) and graph.plan(d, k2) is not graph.plan(d, k)
    torch.autograd.backward(ys, [to_dev(g, gpu) for g in (g0, g1, g2)])
    c2 = ad.case(gname, d, k2, p, mode, 0, ad.SEED, 1.0, k)     # the same x through k2
    same(x.grad, ad.x_grad(c, g0) + ad.x_grad(c, g1) + ad.x_grad(c2, g2),
         f"{vars(E2)}: one x, three maxk_aggregate calls")


# ------------------------------------------------------------------ 5: interleaved lifetimes
@config
@pytest.mark.parametrize("order", [(2, 1, 0), (0, 1, 2), "drop B"], ids=["lifo", "fifo", "drop"])
def test_driver05_interleaved_lifetimes_on_one_plan(gpu, gname, d, k, order):
    """Forward A, B, C with different data (and a different edge_weight tensor each, on the
    weighted plan) on one graph; backward in LIFO order, in FIFO order, and with B's graph
    deleted in between: each gradient is its standalone gradient."""
    graph = ad.shared_graph(gpu, gname)
    for S, E in cases(5, gname, d, k):
        ts = [leaves(S, E, gpu, xvar=v, wvar=v) for v in range(3)]
        outs = [S.fwd(E, graph, t) for t in ts]
        if order == "drop B":
            outs[1] = None
        for v in (0, 2) if order == "drop B" else order:
            backward(outs[v], gouts(S, E, gpu))
            check_grads(S, E, ts[v], refs(S, E, 0, xvar=v, wvar=v),
                        f"call {'ABC'[v]} of order {order}")


# ------------------------------------------------------------------ 6: in-place edits
def _backward_or_inplace_error(outs, gs):
    """True when the backward ran; False when it raised torch's (or the package's) error about
    a tensor modified by an in-place operation. Anything else propagates."""
    try:
        backward(outs, gs)
    except RuntimeError as exc:
        assert "inplace" in str(exc) or "in-place" in str(exc), exc
        return False
    return True


@config
def test_driver06_edits_between_forward_and_backward(gpu, gname, d, k):
    """6a: graph.val edited in place after the forward; 6b: then another forward on the same
    graph (which refreshes the shared plan to the new values) before the first backward. Either
    a RuntimeError about the in-place modification, or the gradient for the values the forward
    ran with; never another. The later call's own gradient is the one for the new values.
    Editing an input after the forward: a surface that saves it raises, every other returns the
    same gradient (only selectors are saved). y.add_() on the outputs changes nothing, except
    for the edge softmax, which saves its output: torch raises."""
    raised = collections.Counter()
    for S, E in cases(6, gname, d, k):
        R = refs(S, E)
        graph = ad.shared_graph(gpu, gname)
        gs = gouts(S, E, gpu)
        for n in S.inputs:                          # an input edited after the forward
            t = leaves(S, E, gpu)
            tin = {m: (v.clone() if v.requires_grad else v) for m, v in t.items()}
            outs = S.fwd(E, graph, tin)
            with torch.no_grad():
                tin[n].mul_(0.0)
            if n in S.saves:
                with pytest.raises(RuntimeError, match=INPLACE):
                    backward(outs, gs)
            else:
                backward(outs, gs)
                check_grads(S, E, t, R, f"{n} zeroed after the forward")
        t = leaves(S, E, gpu)                       # the outputs edited after the forward
        outs = tuple(o.add_(1.0) for o in S.fwd(E, graph, t))
        if S.saves_output:
            with pytest.raises(RuntimeError, match=INPLACE):
                backward(outs, gs)
        else:
            backward(outs, gs)
            check_grads(S, E, t, R, "y.add_() after the forward")
        if not S.uses_graph_val:
            continue
        for req in subsets(S.inputs):               # 6a and 6b
            for later_forward in (False, True):
                own = ad.private_graph(gpu, gname)
                t = leaves(S, E, gpu, req)
                outs = S.fwd(E, own, t)
                own.val.mul_(2.0)
                if later_forward:
                    t2 = leaves(S, E, gpu, req, xvar=1, wvar=1)
                    outs2 = S.fwd(E, own, t2)
                ran = _backward_or_inplace_error(outs, gs)
                raised[(S.name, req, ran)] += 1
                if ran:
                    check_grads(S, E, t, R, f"graph.val edited, later forward {later_forward}, "
                                f"inputs {req}", req)
                if later_forward:
                    backward(outs2, gs)
                    check_grads(S, E, t2, refs(S, E, xvar=1, wvar=1, vscale=2.0),
                                "the later call, on the new values", req)
    mk.clear_plan_cache()
    print("\ndriver 6, graph.val edited: (surface, inputs, backward ran) -> cases",
          dict(raised))


# ------------------------------------------------------------------ 7: create_graph=True
SECOND_ORDER = "differentiate twice|once_differentiable"


@config
def test_driver07_create_graph(gpu, gname, d, k):
    """grad(..., create_graph=True): the first-order values are the plain ones, and they carry
    a node that raises when anything built from them is differentiated, for a constant incoming
    gradient and for one that itself requires grad. A gradient-penalty loss therefore never
    completes a backward that drops the term."""
    graph = ad.shared_graph(gpu, gname)
    for S, E in cases(7, gname, d, k):
        what = f"{S} {vars(E)}"
        t, gs, R = leaves(S, E, gpu), gouts(S, E, gpu), refs(S, E)
        ins = [t[n] for n in S.inputs]
        outs = S.fwd(E, graph, t)
        got = torch.autograd.grad(list(outs), ins, list(gs), create_graph=True)
        for n, g in zip(S.inputs, got):
            same(g, R[n], f"{what} create_graph=True: d/d{n}")
            assert g.requires_grad, f"{what}: d/d{n} came back as a constant"
            with pytest.raises(RuntimeError):       # no path to the inputs, and said so
                torch.autograd.grad(g.sum(), ins)
            with pytest.raises(RuntimeError, match=SECOND_ORDER):
                g.sum().backward()
        for power in (1, 2):                        # constant / differentiable incoming gradient
            t = leaves(S, E, gpu)
            ins = [t[n] for n in S.inputs]
            loss = sum((o ** power * g).sum() for o, g in zip(S.fwd(E, graph, t), gs))
            got = torch.autograd.grad(loss, ins, create_graph=True)
            total = loss + sum(g.pow(2).sum() for g in got)
            with pytest.raises(RuntimeError, match=SECOND_ORDER):
                total.backward()


# ------------------------------------------------------------------ 8: checkpointing
@config
@pytest.mark.parametrize("reentrant", [False, True])
def test_driver08_checkpoint(gpu, gname, d, k, reentrant):
    """torch.utils.checkpoint around the surface, both flavours. The dropout seed of the public
    functions is drawn (seed=None) from torch's CPU generator; both runs start from the same
    torch.manual_seed, the recomputation restores the generator, and the restatement uses the
    seed drawn the same way: gradients equal the plain run's bit for bit, and the restatement."""
    graph = ad.shared_graph(gpu, gname)
    for S, E in cases(8, gname, d, k):
        if E.p and isinstance(S, ad.Agg):
            torch.manual_seed(77 + k)
            drawn = torch.empty((), dtype=torch.int64).random_().item()
            E = env(gname, d, k, E.p, E.mode, seed=drawn, seed_arg=None)
        gs, R = gouts(S, E, gpu), refs(S, E)
        torch.manual_seed(77 + k)
        plain = leaves(S, E, gpu)
        outs = S.fwd(E, graph, plain)
        backward(outs, gs)
        check_grads(S, E, plain, R, "plain run")
        torch.manual_seed(77 + k)
        t = leaves(S, E, gpu)
        names = list(t)
        outs2 = checkpoint(lambda *a: S.fwd(E, graph, dict(zip(names, a))),
                           *[t[n] for n in names], use_reentrant=reentrant)
        for o, o2 in zip(outs, outs2):
            assert torch.equal(o, o2), f"{S} {vars(E)}: checkpointed output differs"
        backward(outs2, gs)
        check_grads(S, E, t, R, f"checkpoint(use_reentrant={reentrant})")
        for n in S.inputs:
            assert torch.equal(t[n].grad, plain[n].grad)


# ------------------------------------------------------------------ 9: no graph
def _plans(S, E, graph, t):
    if isinstance(S, ad.Agg):
        return [graph.weighted_plan(E.d, E.k) if S.weighted else graph.plan(E.d, E.k)]
    if isinstance(S, ad.OpSpGEMM):
        return [ops.get_plan(graph.ptr, graph.idx, t["val"], ad.N, graph.num_edges, E.d, E.k)]
    return []


@config
@pytest.mark.parametrize("mode", [torch.no_grad, torch.inference_mode],
                         ids=["no_grad", "inference_mode"])
def test_driver09_no_graph(gpu, gname, d, k, mode):
    """Under no_grad and inference_mode the outputs are the grad-mode outputs bit for bit and
    have no grad_fn, and the call keeps no plan alive: after clear_plan_cache() and dropping the
    graph a weak reference to the plan is dead while the outputs live. A tensor made in
    inference mode is accepted as a constant input of a later grad-mode call (a surface that
    saves that input refuses it with torch's own error)."""
    for S, E in cases(9, gname, d, k):
        what = f"{S} {vars(E)}"
        graph = ad.shared_graph(gpu, gname)
        ref_outs = S.fwd(E, graph, leaves(S, E, gpu))
        assert all(o.grad_fn is not None for o in ref_outs), what
        lifetime = vars(E) == vars(S.envs(gname, d, k)[0])   # once per surface: it builds plans
        own = ad.private_graph(gpu, gname) if lifetime else graph
        t = leaves(S, E, gpu, req=())
        with mode():
            outs = S.fwd(E, own, t)
        for o, r in zip(outs, ref_outs):
            assert o.grad_fn is None and not o.requires_grad, what
            assert torch.equal(o, r), f"{what}: {mode.__name__} output differs"
        if lifetime:
            alive = [weakref.ref(p) for p in _plans(S, E, own, t)]
            del own, t
            mk.clear_plan_cache()
            gc.collect()
            assert all(r() is None for r in alive), f"{what}: {mode.__name__} kept its plan"
            assert outs[0].shape == ref_outs[0].shape       # the outputs outlive the plan
        if mode is torch.no_grad:
            continue
        with torch.inference_mode():
            const = leaves(S, E, gpu, req=())
        first, rest = S.inputs[0], S.inputs[1:]
        t = dict(const)
        for n in rest:
            t[n] = leaves(S, E, gpu)[n]
        if rest and first in S.saves:
            with pytest.raises(RuntimeError, match="Inference tensors cannot be saved"):
                S.fwd(E, graph, t)
            continue
        outs = S.fwd(E, graph, t)
        for o, r in zip(outs, ref_outs):
            assert torch.equal(o, r), f"{what}: output on an inference-mode input differs"
        if rest:
            backward(outs, gouts(S, E, gpu))
            check_grads(S, E, t, refs(S, E), "inference-mode features, grad-mode weights", rest)
        else:
            assert all(o.grad_fn is None for o in outs), what
    mk.clear_plan_cache()


# ------------------------------------------------------------------ 10: incoming layouts
def _layouts(g, dev):
    """name -> (the gradient tensor in that layout, the dense values it holds)."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    out = {"zero stride": (torch.ones((), device=dev).expand(g.shape), np.ones_like(g))}
    if g.ndim == 1:
        wide = torch.full((g.size + 8,), 7.0, device=dev)
        wide[3:3 + g.size] = to_dev(g, dev)
        out["slice of a longer buffer"] = (wide[3:3 + g.size], g)
        two = torch.full((2 * g.size,), 7.0, device=dev)
        two[::2] = to_dev(g, dev)
        out["every other element"] = (two[::2], g)
        return out
    n, d = g.shape
    out["transposed"] = (to_dev(np.ascontiguousarray(g.T), dev).t(), g)
    wide = torch.full((n, d + 8), 7.0, device=dev)
    wide[:, 3:3 + d] = to_dev(g, dev)
    out["columns of a wider buffer"] = (wide[:, 3:3 + d], g)     # row stride > D, unit columns
    two = torch.full((n, 2 * d), 7.0, device=dev)
    two[:, ::2] = to_dev(g, dev)
    out["every other column"] = (two[:, ::2], g)
    tall = torch.full((3 * n, d), 7.0, device=dev)
    tall[::3] = to_dev(g, dev)
    out["every third row"] = (tall[::3], g)
    return out


def _losses(o, g, dev):
    """name -> (a scalar built from a view of the output, the gradient it sends back)."""
    G = to_dev(g, dev)
    out = {"y.sum()": (o.sum(), np.ones_like(g))}
    m = np.zeros_like(g)
    m[::3] = 1
    out["y[::3]"] = ((o[::3] * G[::3]).sum(), g * m)
    if g.ndim == 2:
        out["y.t()"] = ((o.t() * to_dev(np.ascontiguousarray(g.T), dev)).sum(), g)
        m = np.zeros_like(g)
        m[:, ::2] = 1
        out["y[:, ::2]"] = ((o[:, ::2] * G[:, ::2]).sum(), g * m)
        m = np.zeros_like(g)
        m[:, :g.shape[1] // 2] = 1
        out["y[:, :d // 2]"] = ((o[:, :g.shape[1] // 2] * G[:, :g.shape[1] // 2]).sum(), g * m)
    return out


@config
def test_driver10_incoming_gradient_layouts(gpu, gname, d, k):
    """Gradients that arrive with zero strides, transposed, as columns or rows of a larger
    buffer (both branches of the g_self stride test of the self aggregation), handed over
    directly and produced by autograd from y.sum(), y.t(), y[:, ::2], y[::3], y[:, :d // 2]."""
    graph = ad.shared_graph(gpu, gname)
    for S, E in cases(10, gname, d, k):
        g_np = S.np_gouts(E)
        per_out = [_layouts(g, gpu) for g in g_np]
        for name in per_out[0]:
            t = leaves(S, E, gpu)
            backward(S.fwd(E, graph, t), [lay[name][0] for lay in per_out])
            R = S.ref_grads(E, tuple(lay[name][1] for lay in per_out))
            check_grads(S, E, t, R, f"incoming gradient: {name}")
        t = leaves(S, E, gpu)
        outs = S.fwd(E, graph, t)
        per_out = [_losses(o, g, gpu) for o, g in zip(outs, g_np)]
        for i, name in enumerate(per_out[0]):
            for n in S.inputs:
                t[n].grad = None
            sum(lo[name][0] for lo in per_out).backward(retain_graph=i + 1 < len(per_out[0]))
            R = S.ref_grads(E, tuple(lo[name][1] for lo in per_out))
            check_grads(S, E, t, R, f"loss on {name}")


# ------------------------------------------------------------------ 11: input layouts
def _views(a, dev):
    """name -> (leaf base, the view of it that holds `a`, where the view lies in base)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    out = {}
    if a.ndim == 1:
        base = torch.full((a.size + 8,), 3.0, device=dev)
        base[3:3 + a.size] = to_dev(a, dev)
        out["slice"] = (base, lambda b: b[3:3 + a.size])
        base = torch.full((2 * a.size,), 3.0, device=dev)
        base[::2] = to_dev(a, dev)
        out["strided"] = (base, lambda b: b[::2])
        return out
    n, d = a.shape
    base = torch.full((n, d + 8), 3.0, device=dev)
    base[:, 3:3 + d] = to_dev(a, dev)
    out["base[:, 3:3 + d]"] = (base, lambda b: b[:, 3:3 + d])
    out["base.t()"] = (to_dev(np.ascontiguousarray(a.T), dev), lambda b: b.t())
    return out


@config
def test_driver11_input_layouts(gpu, gname, d, k):
    """The first input as a view of a larger leaf (columns 3 .. 3 + D of a wider buffer; a
    transposed buffer): base.grad holds the restated gradient inside the view and zeros
    outside it. The registered operators keep the reference's "must be contiguous" check: they
    refuse such a view by name, and take its .contiguous() copy."""
    graph = ad.shared_graph(gpu, gname)
    for S, E in cases(11, gname, d, k):
        first = S.inputs[0]
        R = refs(S, E)
        for name, (base, view) in _views(S.np_inputs(E)[first], gpu).items():
            base.requires_grad_(True)
            t = leaves(S, E, gpu)
            t[first] = view(base)
            what = f"{S} {vars(E)} {first} = {name}"
            if not (S.strided_inputs or t[first].is_contiguous()):
                with pytest.raises(RuntimeError, match="contiguous"):
                    S.fwd(E, graph, t)
                t[first] = t[first].contiguous()
            backward(S.fwd(E, graph, t), gouts(S, E, gpu))
            same(view(base.grad).contiguous(), R[first], what)
            outside = base.grad.clone()
            view(outside).zero_()
            assert not outside.any(), f"{what}: gradient outside the view"
            if S.inputs[1:]:
                check_grads(S, E, t, R, what, S.inputs[1:])


# ------------------------------------------------------------------ 12: streams
@config
def test_driver12_forward_on_a_side_stream(gpu, gname, d, k):
    """The forward under torch.cuda.stream(side), the backward called from outside the block
    (autograd runs it on the forward's stream), then one synchronise."""
    graph = ad.shared_graph(gpu, gname)
    side = torch.cuda.Stream(device=gpu)
    for S, E in cases(12, gname, d, k):
        t, gs, R = leaves(S, E, gpu), gouts(S, E, gpu), refs(S, E)
        side.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(side):
            outs = S.fwd(E, graph, t)
        backward(outs, gs)
        torch.cuda.synchronize(gpu)
        check_outs(S, E, outs, "forward on the side stream")
        check_grads(S, E, t, R, "backward after a side-stream forward")


# ------------------------------------------------------------------ (h): the four layers
LAYER_D, LAYER_K, LAYER_P = 64, 16, 0.5
LAYER_CASES = [(kind, train) for kind in ("sage", "gcn", "gin", "gat") for train in (False, True)]
layer_case = pytest.mark.parametrize("kind,train", LAYER_CASES)


def _draw():
    """The seed a fused-dropout call draws from torch's CPU generator (autograd._dropout_pair)."""
    return torch.empty((), dtype=torch.int64).random_().item()


def _layer(kind, dev, train):
    """(layer, its CSRGraph on the sparse sweep graph, f32 features, two upstream gradients)."""
    torch.manual_seed(11)
    kw = dict(maxk=LAYER_K, feat_drop=LAYER_P, fused_dropout=True)
    d = LAYER_D
    layer = {"sage": lambda: mk.MaxKSAGEConv(d, d, "mean", **kw),
             "gcn": lambda: mk.MaxKGCNConv(d, d, norm="both", allow_zero_in_degree=True, **kw),
             "gin": lambda: mk.MaxKGINConv(d, init_eps=0.3, **kw),
             "gat": lambda: mk.MaxKGATConv(d, d, allow_zero_in_degree=True, **kw)}[kind]().to(dev)
    with torch.no_grad():
        for n, prm in layer.named_parameters():
            if n.endswith("bias"):
                prm.uniform_(-0.5, 0.5)
    p, ix, _ = ad.dev_graph(dev, "sparse")
    feat = graphs.features(ad.N, d, seed=3).to(dev)
    G = [graphs.features(ad.N, d, seed=4 + i).to(dev) for i in range(2)]
    return layer.train(train), mk.CSRGraph(p, ix), feat, G


def _layer_ref(kind, layer, csr, feat, G, seed):
    """The f64 dense restatement of one layer call (the formulas of tests/test_layers.py, and
    dglnn.GATConv with one head), with the fused dropout's mask restated from `seed` (None: eval
    mode). The two selections come from the layer's own f32 values: the top-k mask, and the
    leaky_relu branch of each attention score. Returns the output and the gradients of
    `out.backward(G)` by parameter name, "feat" for the features."""
    P = {n: prm.detach().cpu().double().requires_grad_(True)
         for n, prm in layer.named_parameters()}
    f = feat.detach().cpu().double().requires_grad_(True)
    r, c = csr.edge_rows().cpu(), csr.idx.long().cpu()
    with torch.no_grad():
        pre = {"sage": lambda: feat, "gin": lambda: feat, "gcn": lambda: feat @ layer.weight,
               "gat": lambda: layer.fc(feat)}[kind]()
        mask = torch.zeros_like(pre).scatter_(1, pre.topk(LAYER_K, dim=1).indices, 1.0)
        mask = mask.cpu().double()
        if kind == "gat":
            z32 = (pre * layer.attn_l).sum(-1)[csr.idx.long()] + \
                (pre * layer.attn_r).sum(-1)[csr.edge_rows()]
            s = torch.where(z32 > 0, 1.0, layer.negative_slope).cpu().double()
    if seed is not None:
        keep = keep_mask(LAYER_P, seed, np.arange(ad.N)[:, None], np.arange(LAYER_D)[None, :])
        mask = mask * torch.from_numpy(keep * float(drop_scale(LAYER_P)))
    if kind == "sage":
        xm = f * mask
        out = (xm @ P["fc_self.weight"].T + (dense_adj(csr, "mean") @ xm) @ P["fc_neigh.weight"].T
               + P["bias"])
    elif kind == "gcn":
        out = dense_adj(csr, "both") @ ((f @ P["weight"]) * mask) + P["bias"]
    elif kind == "gin":
        xm = f * mask
        out = (1 + P["eps"]) * xm + dense_adj(csr, "sum") @ xm
    else:
        h = f @ P["fc.weight"].T
        e = ((h * P["attn_l"]).sum(-1)[c] + (h * P["attn_r"]).sum(-1)[r]) * s
        top = torch.full((ad.N,), -1e300, dtype=torch.float64).scatter_reduce(
            0, r, e.detach(), "amax")
        pe = (e - top[r]).exp()
        alpha = pe / torch.zeros(ad.N, dtype=torch.float64).index_add_(0, r, pe)[r]
        A = torch.zeros((ad.N, ad.N), dtype=torch.float64).index_put((r, c), alpha,
                                                                     accumulate=True)
        out = A @ (h * mask) + P["bias"]
    out.backward(G.detach().cpu().double())
    grads = {n: v.grad for n, v in P.items()}
    grads["feat"] = f.grad
    return out.detach(), grads


def _assert_close(got, want, what):
    assert got is not None and float(want.abs().max()) > 0, what
    assert close(got, want), (what, float((got.detach().double().cpu() - want).abs().max()),
                              float(want.abs().max()))


@layer_case
def test_layers_driver02_accumulation(gpu, kind, train):
    """Two training steps with different upstream gradients (and, in train mode, the two masks
    of two drawn seeds) and no zero_grad: every .grad is the sum of the two restatements."""
    layer, csr, feat, G = _layer(kind, gpu, train)
    feat.requires_grad_(True)
    torch.manual_seed(5)
    seeds = [_draw(), _draw()] if train else [None, None]
    torch.manual_seed(5)
    for g in G:
        layer(csr, feat).backward(g)
    parts = [_layer_ref(kind, layer, csr, feat, g, s)[1] for g, s in zip(G, seeds)]
    for n, prm in list(layer.named_parameters()) + [("feat", feat)]:
        _assert_close(prm.grad, parts[0][n] + parts[1][n], f"{kind} train={train} {n}.grad")


@layer_case
def test_layers_driver03_partial_gradients(gpu, kind, train):
    """autograd.grad for every non-empty subset of the parameters, the input features constant:
    each result is the matching piece of the full restatement."""
    layer, csr, feat, G = _layer(kind, gpu, train)
    torch.manual_seed(6)
    seed = _draw() if train else None
    want = _layer_ref(kind, layer, csr, feat, G[0], seed)[1]
    named = dict(layer.named_parameters())
    for req in subsets(sorted(named)):
        torch.manual_seed(6)
        got = torch.autograd.grad(layer(csr, feat), [named[n] for n in req], G[0])
        for n, g in zip(req, got):
            _assert_close(g, want[n], f"{kind} train={train} subset {req}: {n}")
        assert all(prm.grad is None for prm in named.values())


@layer_case
def test_layers_driver07_create_graph(gpu, kind, train):
    """create_graph=True through a layer: first-order values as restated, and a penalty on them
    raises in its backward instead of dropping what passes through the kernels' backward."""
    layer, csr, feat, G = _layer(kind, gpu, train)
    feat.requires_grad_(True)
    torch.manual_seed(7)
    seed = _draw() if train else None
    out_ref, want = _layer_ref(kind, layer, csr, feat, G[0], seed)
    named = dict(layer.named_parameters(), feat=feat)
    torch.manual_seed(7)
    out = layer(csr, feat)
    _assert_close(out, out_ref, f"{kind} train={train} output")
    got = torch.autograd.grad(out, list(named.values()), G[0], create_graph=True)
    for n, g in zip(named, got):
        _assert_close(g, want[n], f"{kind} train={train} create_graph=True: {n}")
    total = (out * G[0]).sum() + sum(g.pow(2).sum() for g in got)
    with pytest.raises(RuntimeError, match=SECOND_ORDER):
        total.backward()


@layer_case
@pytest.mark.parametrize("reentrant", [False, True])
def test_layers_driver08_checkpoint(gpu, kind, train, reentrant):
    """checkpoint around the layer, in train mode with fused_dropout=True and a drawn seed: the
    recomputation draws the same seed (checkpoint restores the CPU generator), so output and
    gradients are those of the restatement with that seed's mask."""
    layer, csr, feat, G = _layer(kind, gpu, train)
    feat.requires_grad_(True)
    torch.manual_seed(8)
    seed = _draw() if train else None
    out_ref, want = _layer_ref(kind, layer, csr, feat, G[0], seed)
    torch.manual_seed(8)
    out = checkpoint(layer, csr, feat, use_reentrant=reentrant)
    _assert_close(out, out_ref, f"{kind} train={train} checkpointed output")
    out.backward(G[0])
    for n, prm in list(layer.named_parameters()) + [("feat", feat)]:
        _assert_close(prm.grad, want[n], f"{kind} train={train} reentrant={reentrant} {n}.grad")


# ------------------------------------------------------------------ closure
def test_every_function_and_operator_ran_under_every_driver():
    """Runs last (file order). Every torch.autograd.Function subclass of maxk_kernels.autograd
    and every operator of maxk_kernels.torch_ops with a registered derivative ran under every
    driver, except the pairs autograd_drivers.NOT_APPLICABLE lists with a reason (at most 15 %
    of them). A Function added later fails here until a surface covers it."""
    blocks = {(drv, *c) for drv in ad.DRIVERS for c in CONFIGS}
    if not blocks <= STARTED:
        pytest.skip(f"a -k selection ran {len(STARTED & blocks)} of {len(blocks)} driver blocks")
    names = ad.autograd_functions() + ad.operators_with_derivative()
    pairs = {(n, drv) for n in names for drv in ad.DRIVERS}
    assert set(ad.NOT_APPLICABLE) <= pairs
    assert all(isinstance(r, str) and r for r in ad.NOT_APPLICABLE.values())
    assert len(ad.NOT_APPLICABLE) <= ad.NOT_APPLICABLE_CAP * len(pairs)
    missing = sorted(pairs - RAN - set(ad.NOT_APPLICABLE))
    assert not missing, missing
    print(f"\nautograd drivers: {len(names)} Functions and operators x {len(ad.DRIVERS)} drivers, "
          f"{len(ad.NOT_APPLICABLE)} pairs not applicable; cases per driver: " +
          ", ".join(f"{drv}: {COUNTS[drv]}" for drv in ad.DRIVERS))
