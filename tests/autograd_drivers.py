"""The autograd driver tests' surfaces, inputs and restatements (a plain module, no tests:
tests/test_autograd_driver_inputs.py checks what is built here on the CPU,
tests/test_gpu_autograd_drivers.py drives every surface through every driver on the GPU).

A *surface* is one way a user reaches the kernels through autograd: a public function of
maxk_kernels.autograd or a registered operator of maxk_kernels.torch_ops, with the names of its
differentiable inputs, a forward on device tensors, and numpy restatements of its outputs and of
every input's gradient for any incoming gradient. The restatements are f64 sums on the exactly
summable inputs of tests/sweep.py (integer features and gradients, edge values and edge weights
from {0.5, 1, 2}, dropout scale 2), so every driver compares with np.array_equal; the edge softmax
has no exact inputs and is restated by the two plain `ops` calls, which are deterministic.

Variants give the drivers different data on one graph: `xvar` 0, 1, 2 are the case's features,
their negation and their rows rolled by one; `wvar` picks the edge weights, `gvar` the incoming
gradients.
"""
import functools
import types

import numpy as np
import torch

import maxk_kernels as mk
import sweep
from maxk_kernels import ops
from oracle import oracle
from structured import EXACT_LIMIT, int_features
from test_dropout_capi import drop_scale, dropped_table, keep_mask

N = sweep.N
SEED = sweep.SEED
DK = [(256, 16), (64, 8), (100, 10)]
GRAPHS = ("sparse", "dense")
PS = (0.0, sweep.DROP_P)
MODES = tuple(sweep.MODES)
WEIGHTS = np.array([0.5, 1.0, 2.0], np.float32)
SOFTMAX_RANGE = 16.0
DRIVERS = tuple(range(1, 13))
DEVICE = None                      # set by the GPU module: where the edge softmax is restated


def env(gname, d, k, p=0.0, mode="exact", seed=SEED, seed_arg=SEED):
    """One configuration: `seed` is the dropout seed the restatement uses, `seed_arg` what the
    call is given (None: the call draws it from torch's CPU generator)."""
    return types.SimpleNamespace(gname=gname, d=d, k=k, p=p, mode=mode, seed=seed,
                                 seed_arg=seed_arg)


# ---------------------------------------------------------------------------- inputs
def features(d, k, xvar):
    x = int_features(N, d, seed=1000 + k)
    if xvar == 1:
        return (-x + 0.0).astype(np.float32)
    if xvar == 2:
        return np.ascontiguousarray(np.roll(x, 1, axis=0))
    assert xvar == 0
    return x


def grad_nd(d, k, gvar):
    """Incoming gradient [N, d]: variant 0 is the sweep case's own g."""
    return int_features(N, d, seed=(2000, 4000, 4500)[gvar] + k)


def grad_self(d, k, gvar):
    return int_features(N, d, seed=(3000, 5000, 5500)[gvar] + k)


def grad_nk(k, gvar):
    return int_features(N, k, seed=(6000, 6500, 7000)[gvar] + k)


@functools.lru_cache(maxsize=None)
def weights(gname, wvar):
    rs = np.random.RandomState(700 + wvar)
    return rs.choice(WEIGHTS, sweep.edges(gname)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def edge_rows(gname):
    p = sweep.graph(gname)[0]
    return np.repeat(np.arange(N), np.diff(p))


@functools.lru_cache(maxsize=None)
def logits(gname, xvar):
    return (np.random.default_rng(5 + xvar).random(sweep.edges(gname)) *
            SOFTMAX_RANGE).astype(np.float32)


def grad_edges(gname, gvar):
    return np.random.default_rng(31 + gvar).standard_normal(sweep.edges(gname)).astype(np.float32)


# ---------------------------------------------------------------------------- exact cases
@functools.lru_cache(maxsize=256)
def case(gname, d, k, p=0.0, mode="exact", xvar=0, seed=SEED, vscale=1.0, xk=None):
    """The top-k side of one exact case on a sweep graph, built as structured.exact_case builds
    it: features, the oracle's table and selectors, the dropped table, and which slots are filled
    (ref_compat fills min(#(x > pivot), k) slots and pads the rest with (0.0f, 0)). `vscale`
    scales the graph's edge values (an in-place edit of graph.val); `xk`: the features are those
    of the case with that k (one x through two different k)."""
    pt, ix, v = sweep.graph(gname)
    v = (v * np.float32(vscale)).astype(np.float32)
    x = features(d, k if xk is None else xk, xvar)
    od0, oi = oracle.maxk(x, k, mode)
    count = sweep.topk_counts(x, k, mode)
    filled = np.arange(k)[None, :] < count[:, None]
    od = dropped_table(od0, oi, p, seed) if p else od0
    scale = float(drop_scale(p)) if p else 1.0
    keep = (keep_mask(p, seed, np.arange(N)[:, None], oi) if p
            else np.ones(oi.shape, bool))
    rows = np.repeat(np.arange(N)[:, None], k, 1)
    return types.SimpleNamespace(p=pt, ix=ix, v=v, d=d, k=k, x=x, od0=od0, od=od, oi=oi,
                                 count=count, filled=filled, keep=keep, scale=scale, rows=rows,
                                 drop_p=p, gname=gname)


def C(E, xvar=0, vscale=1.0):
    return case(E.gname, E.d, E.k, E.p, E.mode, xvar, E.seed, vscale)


def scatter(c, t):
    """The MaxK scatter of a per-slot gradient t [N, k] (f64): filled slots only, through the
    dropout mask and scale."""
    out = np.zeros((N, c.d), np.float64)
    f = c.filled
    out[c.rows[f], c.oi[f]] = (np.asarray(t, np.float64) * c.keep * c.scale)[f]
    return out


def sspmm(c, g, v=None):
    """(A^T g sampled at the selectors [N, k], its magnitude), f64 sums."""
    return oracle.sspmm_backward(c.p, c.ix, c.v if v is None else v,
                                 np.ascontiguousarray(g, dtype=np.float32), c.oi, with_mag=True)


def forward(c, v=None):
    return oracle.spgemm_forward(c.p, c.ix, c.v if v is None else v, c.od, c.oi, c.d,
                                 with_mag=True)


def dense_row(c):
    """x_m = dropout(x * topk_mask(x)) dense."""
    out = np.zeros((N, c.d), np.float32)
    out[c.rows[c.filled], c.oi[c.filled]] = c.od[c.filled]
    return out


def x_grad(c, g_agg=None, g_self=None, g_slots=None, v=None, mag=False):
    """x.grad of any MaxK surface: per slot, the SSpMM of the aggregated output's gradient, plus
    the dense output's gradient at the slot's feature, plus the table's own gradient; scattered.
    `mag`: the same with absolute values (the sum of |terms|)."""
    t = np.zeros((N, c.k), np.float64)
    if g_agg is not None:
        t = t + sspmm(c, g_agg, v)[1 if mag else 0]
    if g_self is not None:
        s = np.asarray(g_self, np.float64)[c.rows, c.oi]
        t = t + (np.abs(s) if mag else s)
    if g_slots is not None:
        s = np.asarray(g_slots, np.float64)
        t = t + (np.abs(s) if mag else s)
    if mag:
        out = np.zeros((N, c.d), np.float64)
        out[c.rows[c.filled], c.oi[c.filled]] = (t * c.scale)[c.filled]
        return out
    return scatter(c, t)


def edge_value_grad(c, g, mag=False):
    """d loss / d val [E] of the SpGEMM: sum_l table[c, l] * g[r, selector[c, l]] per edge."""
    r = edge_rows(c.gname)
    t = c.od[c.ix].astype(np.float64) * np.asarray(g, np.float64)[r[:, None], c.oi[c.ix]]
    return np.abs(t).sum(1) if mag else t.sum(1)


def dense_forward(gname, x, v, mag=False):
    p, ix, _ = sweep.graph(gname)
    t = v[:, None].astype(np.float64) * np.asarray(x, np.float64)[ix]
    out = np.zeros((N, x.shape[1]), np.float64)
    np.add.at(out, edge_rows(gname), np.abs(t) if mag else t)
    return out


def dense_x_grad(gname, g, v, mag=False):
    p, ix, _ = sweep.graph(gname)
    t = v[:, None].astype(np.float64) * np.asarray(g, np.float64)[edge_rows(gname)]
    out = np.zeros((N, g.shape[1]), np.float64)
    np.add.at(out, ix, np.abs(t) if mag else t)
    return out


def dense_value_grad(gname, x, g, mag=False):
    p, ix, _ = sweep.graph(gname)
    t = np.asarray(x, np.float64)[ix] * np.asarray(g, np.float64)[edge_rows(gname)]
    return np.abs(t).sum(1) if mag else t.sum(1)


def f32(a):
    return None if a is None else np.asarray(a).astype(np.float32)


# ---------------------------------------------------------------------------- device side
def to_dev(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


@functools.lru_cache(maxsize=None)
def dev_graph(dev, gname):
    p, ix, v = sweep.graph(gname)
    return to_dev(p, dev), to_dev(ix, dev), to_dev(v, dev)


@functools.lru_cache(maxsize=None)
def shared_graph(dev, gname):
    """One CSRGraph per sweep graph, shared by the drivers (and so are its plans)."""
    return mk.CSRGraph(*dev_graph(dev, gname))


def private_graph(dev, gname):
    """A CSRGraph with edge values of its own, for the drivers that edit them."""
    p, ix, v = dev_graph(dev, gname)
    return mk.CSRGraph(p, ix, v.clone())


# ---------------------------------------------------------------------------- surfaces
class Surface:
    """See the module docstring. `covers`: the Function classes (by name) or operators
    (`maxk::name`) the forward and backward run. `saves`: inputs that the surface saves for the
    backward when every input needs a gradient. `plan`: whether a call holds a GraphPlan."""
    name = ""
    covers = ()
    inputs = ("x",)
    takes_mode = takes_drop = True
    exact = True
    uses_graph_val = True
    saves = ()
    plan = True
    saves_output = False
    strided_inputs = True        # False: the surface refuses a non-contiguous input

    def __repr__(self):
        return self.name

    def envs(self, gname, d, k):
        return [env(gname, d, k, p, m)
                for p in (PS if self.takes_drop else PS[:1])
                for m in (MODES if self.takes_mode else MODES[:1])]


class Agg(Surface):
    """(a) maxk -> spgemm, (b) maxk_aggregate, (c) maxk_self_aggregate, and (d) each with
    edge_weight=."""

    def __init__(self, form, weighted):
        self.form, self.weighted = form, weighted
        base = {"spgemm": "maxk+spgemm", "aggregate": "maxk_aggregate",
                "self": "maxk_self_aggregate"}[form]
        self.name = base + ("+edge_weight" if weighted else "")
        fn = "EdgeWeightedFunction" if weighted else {
            "spgemm": "SpGEMMFunction", "aggregate": "MaxKAggregateFunction",
            "self": "MaxKSelfAggregateFunction"}[form]
        self.covers = (("MaxKFunction",) if form == "spgemm" else ()) + (fn,)
        self.inputs = ("x", "w") if weighted else ("x",)

    def np_inputs(self, E, xvar=0, wvar=0):
        t = {"x": C(E, xvar).x}
        if self.weighted:
            t["w"] = weights(E.gname, wvar)
        return t

    def fwd(self, E, graph, t):
        kw = dict(dropout_p=E.p, seed=E.seed_arg)
        ew = dict(edge_weight=t["w"]) if self.weighted else {}
        if self.form == "spgemm":
            sp, si = mk.maxk(t["x"], E.k, E.mode, **kw)
            return (mk.spgemm(sp, si, graph, E.d, **ew),)
        if self.form == "aggregate":
            return (mk.maxk_aggregate(t["x"], graph, E.k, E.mode, **kw, **ew),)
        return tuple(mk.maxk_self_aggregate(t["x"], graph, E.k, E.mode, **kw, **ew))

    def np_gouts(self, E, gvar=0):
        g = (grad_nd(E.d, E.k, gvar),)
        return (grad_self(E.d, E.k, gvar),) + g if self.form == "self" else g

    def _v(self, c, E, wvar):
        return c.v * weights(E.gname, wvar) if self.weighted else c.v

    def ref_outs(self, E, xvar=0, wvar=0, vscale=1.0):
        c = C(E, xvar, vscale)
        y = (f32(forward(c, self._v(c, E, wvar))[0]),)
        return (dense_row(c),) + y if self.form == "self" else y

    def ref_grads(self, E, gouts, xvar=0, wvar=0, vscale=1.0, mag=False):
        c = C(E, xvar, vscale)
        g_agg = gouts[-1]
        g_self = gouts[0] if self.form == "self" else None
        r = {"x": x_grad(c, g_agg, g_self, v=self._v(c, E, wvar), mag=mag)}
        if self.weighted:
            gv = (edge_value_grad(c, g_agg, mag) if g_agg is not None
                  else np.zeros(c.ix.size))
            r["w"] = gv * c.v
        return r


class Dense(Surface):
    """(e) dense_aggregate, with and without edge_weight."""
    takes_mode = takes_drop = False
    plan = False

    def __init__(self, weighted):
        self.weighted = weighted
        self.name = "dense_aggregate" + ("+edge_weight" if weighted else "")
        self.covers = ("DenseEdgeWeightedFunction" if weighted else "DenseAggFunction",)
        self.inputs = ("x", "w") if weighted else ("x",)
        self.saves = ("x",) if weighted else ()

    def np_inputs(self, E, xvar=0, wvar=0):
        t = {"x": features(E.d, E.k, xvar)}
        if self.weighted:
            t["w"] = weights(E.gname, wvar)
        return t

    def fwd(self, E, graph, t):
        return (mk.dense_aggregate(t["x"], graph, t["w"] if self.weighted else None),)

    def np_gouts(self, E, gvar=0):
        return (grad_nd(E.d, E.k, gvar),)

    def _v(self, E, wvar, vscale):
        v = (sweep.graph(E.gname)[2] * np.float32(vscale)).astype(np.float32)
        return v, (v * weights(E.gname, wvar) if self.weighted else v)

    def ref_outs(self, E, xvar=0, wvar=0, vscale=1.0):
        return (f32(dense_forward(E.gname, features(E.d, E.k, xvar),
                                  self._v(E, wvar, vscale)[1])),)

    def ref_grads(self, E, gouts, xvar=0, wvar=0, vscale=1.0, mag=False):
        v, ve = self._v(E, wvar, vscale)
        r = {"x": dense_x_grad(E.gname, gouts[0], ve, mag)}
        if self.weighted:
            r["w"] = dense_value_grad(E.gname, features(E.d, E.k, xvar), gouts[0], mag) * v
        return r


class Softmax(Surface):
    """(f) edge_softmax, and the operator. Not exact: restated by the plain `ops` calls on the
    device (deterministic, test_repeated_calls_are_bitwise_equal), which
    test_gpu_autograd_drivers holds to the float64 bounds of test_gpu_edge_softmax once."""
    inputs = ("logits",)
    takes_mode = takes_drop = False
    exact = False
    uses_graph_val = False
    plan = False
    saves_output = True

    def __init__(self, op):
        self.op = op
        self.name = "op.edge_softmax" if op else "edge_softmax"
        self.covers = ("maxk::edge_softmax",) if op else ("EdgeSoftmaxFunction",)
        self.strided_inputs = not op

    def np_inputs(self, E, xvar=0, wvar=0):
        return {"logits": logits(E.gname, xvar)}

    def fwd(self, E, graph, t):
        if self.op:
            return (torch.ops.maxk.edge_softmax(graph.ptr, t["logits"]),)
        return (mk.edge_softmax(graph, t["logits"]),)

    def np_gouts(self, E, gvar=0):
        return (grad_edges(E.gname, gvar),)

    def ref_outs(self, E, xvar=0, wvar=0, vscale=1.0):
        ptr = dev_graph(DEVICE, E.gname)[0]
        return (ops.edge_softmax(ptr, to_dev(logits(E.gname, xvar), DEVICE)).cpu().numpy(),)

    def ref_grads(self, E, gouts, xvar=0, wvar=0, vscale=1.0, mag=False):
        ptr = dev_graph(DEVICE, E.gname)[0]
        y = ops.edge_softmax(ptr, to_dev(logits(E.gname, xvar), DEVICE))
        g = to_dev(np.ascontiguousarray(gouts[0], dtype=np.float32), DEVICE)
        return {"logits": ops.edge_softmax_backward(ptr, y, g).cpu().numpy()}


class OpMaxK(Surface):
    """(g) torch.ops.maxk.maxk_forward / maxk_dropout_forward / maxk_dense_forward."""
    takes_mode = False
    uses_graph_val = False
    plan = False
    strided_inputs = False

    def __init__(self, kind):
        self.kind = kind
        self.name = f"op.maxk_{kind}_forward" if kind != "plain" else "op.maxk_forward"
        self.covers = ("maxk::" + self.name[3:],)
        self.takes_drop = kind != "plain"

    def np_inputs(self, E, xvar=0, wvar=0):
        return {"x": C(E, xvar).x}

    def fwd(self, E, graph, t):
        if self.kind == "plain":
            return (torch.ops.maxk.maxk_forward(t["x"], E.k)[0],)
        if self.kind == "dropout":
            return (torch.ops.maxk.maxk_dropout_forward(t["x"], E.k, E.p, E.seed)[0],)
        return tuple(torch.ops.maxk.maxk_dense_forward(t["x"], E.k, E.p, E.seed)[:2])

    def np_gouts(self, E, gvar=0):
        g = (grad_nk(E.k, gvar),)
        return (grad_self(E.d, E.k, gvar),) + g if self.kind == "dense" else g

    def ref_outs(self, E, xvar=0, wvar=0, vscale=1.0):
        c = C(E, xvar)
        return (dense_row(c), c.od) if self.kind == "dense" else (c.od,)

    def ref_grads(self, E, gouts, xvar=0, wvar=0, vscale=1.0, mag=False):
        g_self = gouts[0] if self.kind == "dense" else None
        return {"x": x_grad(C(E, xvar), None, g_self, gouts[-1], mag=mag)}


class OpSpGEMM(Surface):
    """(g) torch.ops.maxk.spgemm_forward: differentiable in the table and in the edge values,
    which it takes as a tensor (`wvar` picks them: graph values times a weight variant)."""
    name = "op.spgemm_forward"
    covers = ("maxk::spgemm_forward",)
    inputs = ("sp_data", "val")
    takes_mode = takes_drop = False
    uses_graph_val = False       # the values are its own input: editing them is an input edit
    strided_inputs = False
    saves = ("sp_data", "val")

    def _val(self, E, wvar, vscale=1.0):
        return (sweep.graph(E.gname)[2] * weights(E.gname, wvar) *
                np.float32(vscale)).astype(np.float32)

    def np_inputs(self, E, xvar=0, wvar=0):
        c = C(E, xvar)
        return {"sp_data": c.od, "val": self._val(E, wvar), "si": c.oi}   # si: a constant

    def fwd(self, E, graph, t):
        return (torch.ops.maxk.spgemm_forward(graph.ptr, graph.idx, t["val"], t["sp_data"],
                                              t["si"], N, graph.num_edges, E.k, E.d),)

    def np_gouts(self, E, gvar=0):
        return (grad_nd(E.d, E.k, gvar),)

    def ref_outs(self, E, xvar=0, wvar=0, vscale=1.0):
        c = C(E, xvar)
        return (f32(forward(c, self._val(E, wvar, vscale))[0]),)

    def ref_grads(self, E, gouts, xvar=0, wvar=0, vscale=1.0, mag=False):
        c = C(E, xvar)
        return {"sp_data": sspmm(c, gouts[0], self._val(E, wvar, vscale))[1 if mag else 0],
                "val": edge_value_grad(c, gouts[0], mag)}


SURFACES = ([Agg(form, False) for form in ("spgemm", "aggregate", "self")] +
            [Agg(form, True) for form in ("spgemm", "aggregate", "self")] +
            [Dense(False), Dense(True), Softmax(False),
             OpMaxK("plain"), OpMaxK("dropout"), OpMaxK("dense"), OpSpGEMM(), Softmax(True)])
BY_NAME = {s.name: s for s in SURFACES}


# ---------------------------------------------------------------------------- closure
def autograd_functions():
    """Names of the torch.autograd.Function subclasses defined in maxk_kernels.autograd."""
    from maxk_kernels import autograd
    return sorted(n for n, v in vars(autograd).items()
                  if isinstance(v, type) and issubclass(v, torch.autograd.Function) and
                  v.__module__ == autograd.__name__)


def operators_with_derivative():
    """Qualified names of the operators of maxk_kernels.torch_ops that registered a derivative."""
    from torch._library.custom_ops import CustomOpDef

    from maxk_kernels import torch_ops
    return sorted({v._qualname for v in vars(torch_ops).values()
                   if isinstance(v, CustomOpDef) and v._backward_fn is not None})


# (covered name, driver) pairs that do not apply, each with its reason. The closure test allows at
# most NOT_APPLICABLE_CAP of all pairs here.
NOT_APPLICABLE = {}
NOT_APPLICABLE_CAP = 0.15


def exact_sum_ok(mag, terms=4, quantum=0.5):
    """Whether sums of up to `terms` gradients whose own sums of |terms| are `mag` stay exact in
    f32 in any order: multiples of `quantum` below 2^24 * quantum. structured.EXACT_LIMIT is that
    bound's half for quantum 0.5 (partial sums below 2^23)."""
    m = np.asarray(mag, np.float64)
    return bool(np.isfinite(m).all() and terms * float(m.max(initial=0.0)) <=
                EXACT_LIMIT * (quantum / 0.5))
