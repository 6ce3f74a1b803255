"""What the fused MaxK aggregation Functions call, with which arguments, and what they save.

CPU part: the MaxK input-gradient logic (``autograd._maxk_input_grad``: the zero table, the
padding repointing, the in-place-rows test, the scatter call, the empty-row fill) on CPU tensors,
with ``ops.maxk_backward`` replaced by a recording fake; and ``ops._rows_in_place`` directly.

GPU part: ``maxk_aggregate`` and ``maxk_self_aggregate``, each with and without ``edge_weight=``,
under spies that call through. The sequence of calls into ``ops`` and the plan, with the optional
arguments each call was given, is held to a table written out from the Functions as they stood
before they shared one forward and one backward; so are the saved tensors, and the three
Functions' aggregated output and input gradient are held bit for bit to each other."""
import inspect

import numpy as np
import pytest
import torch

import maxk_kernels as mk
from maxk_kernels import autograd, graphs, ops


def input_grad(grad_sp, sp_index, count, dim_origin, dropout, g_self):
    return autograd._maxk_input_grad(grad_sp, sp_index, count, dim_origin, dropout, g_self)


rows_in_place = ops._rows_in_place


# ------------------------------------------------------------------ CPU: the input gradient
N, K, D = 6, 3, 8
COUNTS = [3, 1, 0, 2, 3, 0]
SP_INDEX = [[1, 4, 6], [2, 0, 0], [0, 0, 0], [3, 5, 0], [0, 2, 7], [0, 0, 0]]


class FakeScatter:
    """Stands in for ``ops.maxk_backward``: records its arguments, returns a constant ``[N, D]``
    tensor. The constant is 0 except where a test has to see which rows were filled with 0
    afterwards, which a result of zeros could not show."""

    def __init__(self, fill=0.0):
        self.fill, self.calls = fill, []

    def __call__(self, grad_output, indices, dim_origin=None, dropout=None, grad_dense=None):
        self.calls.append(dict(grad_output=grad_output, indices=indices, dim_origin=dim_origin,
                               dropout=dropout, grad_dense=grad_dense))
        return torch.full((indices.shape[0], dim_origin), self.fill)


@pytest.fixture
def scatter(monkeypatch):
    fake = FakeScatter()
    monkeypatch.setattr(ops, "maxk_backward", fake)
    return fake


def _tables():
    sp_index = torch.tensor(SP_INDEX, dtype=torch.uint8)
    count = torch.tensor(COUNTS, dtype=torch.int32)
    grad_sp = torch.arange(1, N * K + 1, dtype=torch.float32).reshape(N, K)
    return grad_sp, sp_index, count


def _masked(grad_sp, sp_index):
    """The tables the scatter must receive for COUNTS, written out slot by slot."""
    g, i = grad_sp.clone(), sp_index.clone()
    g[1, 1:], i[1, 1:] = grad_sp[1, 0], sp_index[1, 0]
    g[3, 2], i[3, 2] = grad_sp[3, 1], sp_index[3, 1]
    for r in (2, 5):        # no filled slot: selector of slot 0, gradient 0
        g[r, :], i[r, :] = 0.0, sp_index[r, 0]
    return g, i


def test_no_count_passes_the_tables_through(scatter):
    grad_sp, sp_index, _ = _tables()
    out = input_grad(grad_sp, sp_index, None, D, (0.5, 7), None)
    (call,) = scatter.calls
    assert call["grad_output"] is grad_sp and call["indices"] is sp_index
    assert call["dim_origin"] == D and call["dropout"] == (0.5, 7) and call["grad_dense"] is None
    assert out.shape == (N, D)
    # only the dense output had a gradient, exact mode: no table at all
    g_self = torch.ones(N, D)
    input_grad(None, sp_index, None, D, None, g_self)
    call = scatter.calls[1]
    assert call["grad_output"] is None and call["grad_dense"] is g_self
    assert call["dropout"] is None


def test_absent_aggregate_gradient_with_a_count_is_a_zero_table(scatter):
    _, sp_index, count = _tables()
    input_grad(None, sp_index, count, D, None, torch.ones(N, D))
    (call,) = scatter.calls
    got = call["grad_output"]
    assert got.shape == (N, K) and got.dtype == torch.float32 and got.is_contiguous()
    assert not got.any()
    assert torch.equal(call["indices"], _masked(torch.zeros(N, K), sp_index)[1])


@pytest.mark.parametrize("with_self", [False, True])
def test_padding_slots_point_at_the_last_filled_slot(scatter, with_self):
    grad_sp, sp_index, count = _tables()
    g_self = torch.ones(N, D) if with_self else None
    input_grad(grad_sp, sp_index, count, D, None, g_self)
    (call,) = scatter.calls
    want_g, want_i = _masked(grad_sp, sp_index)
    assert torch.equal(call["grad_output"], want_g) and torch.equal(call["indices"], want_i)
    assert call["grad_output"].is_contiguous() and call["indices"].is_contiguous()
    assert call["indices"].dtype == torch.uint8 and call["grad_dense"] is g_self


@pytest.mark.parametrize("with_self", [False, True])
def test_rows_that_filled_no_slot_are_zeroed_exactly_with_a_dense_gradient(monkeypatch,
                                                                           with_self):
    fake = FakeScatter(fill=1.0)
    monkeypatch.setattr(ops, "maxk_backward", fake)
    grad_sp, sp_index, count = _tables()
    out = input_grad(grad_sp, sp_index, count, D, None, torch.ones(N, D) if with_self else None)
    want = torch.ones(N, D)
    if with_self:
        want[[2, 5]] = 0.0
    assert torch.equal(out, want)
    # without a count every row filled k slots
    out = input_grad(grad_sp, sp_index, None, D, None, torch.ones(N, D) if with_self else None)
    assert torch.equal(out, torch.ones(N, D))


@pytest.mark.parametrize("with_count", [False, True])
def test_dense_gradient_with_strided_rows_is_not_copied(scatter, with_count):
    grad_sp, sp_index, count = _tables()
    buf = torch.arange(N * (D + 4), dtype=torch.float32).reshape(N, D + 4)
    g_self = buf[:, :D]
    assert g_self.stride() == (D + 4, 1) and not g_self.is_contiguous()
    input_grad(grad_sp, sp_index, count if with_count else None, D, None, g_self)
    got = scatter.calls[0]["grad_dense"]
    assert got.data_ptr() == buf.data_ptr() and got.stride() == (D + 4, 1)
    assert got.shape == (N, D)


@pytest.mark.parametrize("with_count", [False, True])
def test_transposed_dense_gradient_arrives_contiguous(scatter, with_count):
    grad_sp, sp_index, count = _tables()
    g_self = torch.arange(N * D, dtype=torch.float32).reshape(D, N).t()
    assert g_self.shape == (N, D) and g_self.stride() == (1, N)
    input_grad(grad_sp, sp_index, count if with_count else None, D, None, g_self)
    got = scatter.calls[0]["grad_dense"]
    assert got.is_contiguous() and torch.equal(got, g_self)


def test_rows_in_place():
    t = torch.arange(48, dtype=torch.float32).reshape(6, 8)
    assert rows_in_place(t) is t                                     # contiguous
    strided = torch.zeros(6, 12)[:, :8]
    assert rows_in_place(strided) is strided                         # strided rows
    cols = torch.arange(96, dtype=torch.float32).reshape(6, 16)[:, ::2]
    got = rows_in_place(cols)                                        # non-unit column stride
    assert got.is_contiguous() and torch.equal(got, cols)
    expanded = torch.arange(8, dtype=torch.float32)[None, :].expand(6, 8)
    assert expanded.stride() == (0, 1)
    got = rows_in_place(expanded)                                    # rows on top of each other
    assert got.is_contiguous() and torch.equal(got, expanded)
    for stride in (0, 3, 8, 11):                                     # one row: any row stride
        one = torch.as_strided(torch.arange(8, dtype=torch.float32), (1, 8), (stride, 1))
        assert rows_in_place(one) is one
    one = torch.as_strided(torch.arange(16, dtype=torch.float32), (1, 8), (3, 2))
    got = rows_in_place(one)                                         # ... but unit columns
    assert got.is_contiguous() and torch.equal(got, one)
    flat = torch.arange(16, dtype=torch.float32)[::2]
    got = rows_in_place(flat)                                        # 1-D: made contiguous
    assert got.dim() == 1 and got.is_contiguous() and torch.equal(got, flat)


# ------------------------------------------------------------------ GPU: the call trace
N_G, D_G, K_G, SEED_G = 40, 64, 8, 1234
FORMS = ("aggregate", "self")


def _flags(args, names, truths=()):
    return tuple([n for n in names if args.get(n) is not None] + [n for n in truths if args[n]])


FLAGS = {
    "maxk_forward": lambda a: _flags(a, ("records", "out", "dense", "stats", "dropout"),
                                     ("return_values", "return_count")),
    "maxk_backward": lambda a: _flags(a, ("grad_dense", "dropout")) + (
        ("grad_output is None",) if a["grad_output"] is None else ()),
    "spgemm_edge_grad": lambda a: _flags(a, ("out",)),
    "forward": lambda a: _flags(a, ("out", "stats")),
    "forward_records": lambda a: _flags(a, ("out", "stats")),
    "backward": lambda a: _flags(a, ("grad_sp",)),
    "refresh_values": lambda a: (),
}


@pytest.fixture
def trace(monkeypatch):
    """Spies that call through; each call is logged as ``(name, flags)``."""
    log = []

    def spy(owner, name):
        real = getattr(owner, name)
        sig = inspect.signature(real)

        def wrapper(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            log.append((name, tuple(sorted(FLAGS[name](bound.arguments)))))
            return real(*args, **kwargs)

        monkeypatch.setattr(owner, name, wrapper)

    for name in ("maxk_forward", "maxk_backward", "spgemm_edge_grad"):
        spy(ops, name)
    for name in ("forward", "forward_records", "backward", "refresh_values"):
        spy(ops.GraphPlan, name)
    return log


def expected_trace(form, weighted, w_grad, mode, drop, grads, records, fixed):
    """The calls of one forward and backward, in order, as the Functions made them before they
    shared one forward and one backward. ``grads``: which outputs get a gradient."""
    count = mode == "ref_compat"
    topk = {"records" if records else "out"}
    if fixed:
        topk.add("stats")           # the pair only for a fixed-point forward
    if count:
        topk.add("return_count")
    if drop:
        topk.add("dropout")
    if form == "self":
        topk.add("dense")
    # the [N, k] value table: never next to records without edge weights; with them only when
    # the values need a gradient. A plan that gathers plain tables always gets both.
    if not records or (weighted and w_grad):
        topk.add("return_values")
    stats = ("stats",) if fixed else ()
    seq = [("refresh_values", ())] if weighted else []
    seq += [("maxk_forward", tuple(sorted(topk))),
            ("forward_records" if records else "forward", stats)]
    g_agg, g_self = grads in ("agg", "both"), grads in ("dense", "both")
    if g_agg and weighted and w_grad:
        seq.append(("spgemm_edge_grad", ()))
    if g_agg:                       # the snapshot is this call's own: no second refresh
        seq.append(("backward", ()))
    scatter = set()
    if g_self:
        scatter.add("grad_dense")
    if drop:
        scatter.add("dropout")
    if not g_agg and not count:     # ref_compat scatters a zero table instead
        scatter.add("grad_output is None")
    seq.append(("maxk_backward", tuple(sorted(scatter))))
    return seq


def expected_saved(weighted, w_grad, mode):
    saved = [((N_G, K_G), torch.uint8)]
    if mode == "ref_compat":
        saved.append(((N_G,), torch.int32))
    if weighted and w_grad:
        saved.append(((N_G, K_G), torch.float32))
    return saved


@pytest.fixture(scope="module")
def trace_graph(gpu):
    """40 nodes; row 0 has no edge, row 1 has 24, the others 1 to 6.

    The SSpMM adds a column's terms into f32 accumulators in the order its waves arrive, so two
    backwards agree bit for bit only where every sum is exact in any order (see
    test_gpu_edge_grad.py). Hence edge values in {0.5, 1, 2} and upstream gradients in
    {-2 .. 2}: a column's sum over at most 40 in-edges is a multiple of 0.5 below 2^8, also after
    the dropout factor 2. The features are multiples of 2^-10 below 2^3, so the forward's sums
    (at most 24 terms) are exact too, and those with a 1e6 entry in the f64 the k = 8 forward
    accumulates in."""
    rng = np.random.default_rng(40)
    deg = rng.integers(1, 7, size=N_G)
    deg[0], deg[1] = 0, 24
    ptr = np.zeros(N_G + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(deg)
    idx = np.concatenate([np.sort(rng.choice(N_G, size=int(c), replace=False)) for c in deg])
    val = rng.choice(np.array([0.5, 1.0, 2.0], dtype=np.float32), size=idx.size)
    graph = mk.CSRGraph(torch.from_numpy(ptr).to(gpu), torch.from_numpy(idx).to(gpu),
                        torch.from_numpy(val).to(gpu))
    assert graph.in_degrees()[0] == 0 and graph.in_degrees()[1] >= 20
    x = (graphs.features(N_G, D_G, seed=41) * 1024).round().clamp(-8191, 8191) / 1024
    x[3, :] = 1.0           # ref_compat: a constant row fills no slot
    x[::7, 5] = 1e6         # ref_compat: rows with one filled slot and padding
    g_agg = torch.from_numpy(rng.integers(-2, 3, size=(N_G, D_G)).astype(np.float32)).to(gpu)
    g_self = graphs.features(N_G, D_G, seed=43).to(gpu)
    return graph, x.to(gpu), g_agg, g_self


def _run(form, graph, x0, mode, p, grads, g_agg, g_self, weight=None):
    """One forward and backward: (agg, x.grad, saved shapes and dtypes, weight)."""
    x = x0.clone().requires_grad_(True)
    fn = mk.maxk_aggregate if form == "aggregate" else mk.maxk_self_aggregate
    out = fn(x, graph, K_G, mode, dropout_p=p, seed=SEED_G, edge_weight=weight)
    x_m, agg = out if form == "self" else (None, out)
    saved = [(tuple(t.shape), t.dtype) for t in agg.grad_fn.saved_tensors]
    if grads == "both":
        torch.autograd.backward([x_m, agg], [g_self, g_agg])
    elif grads == "agg":
        agg.backward(g_agg)
    else:
        x_m.backward(g_self)
    return agg.detach(), x.grad, saved


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("mode", ["exact", "ref_compat"])
@pytest.mark.parametrize("records", [True, False])
def test_call_trace_saved_tensors_and_bit_identity(gpu, trace_graph, trace, monkeypatch,
                                                   records, mode, p):
    graph, x0, g_agg, g_self = trace_graph
    plan = graph.plan(D_G, K_G)
    assert plan.new_records() is not None       # the default plan at k = 8 gathers records
    if not records:                             # ... the plain-table branch: no records to take
        monkeypatch.setattr(ops.GraphPlan, "new_records", lambda self: None)
    fixed = plan.fwd_fixed
    assert graph.weighted_plan(D_G, K_G).fwd_fixed == fixed
    del trace[:]
    same_agg, same_grad = [], []
    for form in FORMS:
        for weighted in (False, True):
            for w_grad in ((False, True) if weighted else (False,)):
                for grads in (("agg", "dense", "both") if form == "self" else ("agg",)):
                    w = None
                    if weighted:
                        w = torch.ones(graph.num_edges, device=gpu).requires_grad_(w_grad)
                    agg, grad_x, saved = _run(form, graph, x0, mode, p, grads, g_agg, g_self, w)
                    case = (form, weighted, w_grad, grads)
                    assert trace == expected_trace(form, weighted, w_grad, mode, p > 0, grads,
                                                   records, fixed), case
                    del trace[:]
                    assert saved == expected_saved(weighted, w_grad, mode), case
                    if weighted:    # the edge gradient only from the aggregated output
                        assert (w.grad is not None) == (w_grad and grads != "dense"), case
                    same_agg.append(agg)
                    if grads == "agg":
                        same_grad.append(grad_x)
    assert len(same_agg) == 12 and len(same_grad) == 6
    for other in same_agg[1:]:
        assert torch.equal(other.view(torch.int32), same_agg[0].view(torch.int32))
    for other in same_grad[1:]:
        assert torch.equal(other.view(torch.int32), same_grad[0].view(torch.int32))
    assert bool(same_grad[0].any()) and bool(same_agg[0][1].any())
    assert not bool(same_agg[0][0].any())       # the row without edges
