"""GPU: maxk_sddmm_edge_grad, the gradient of the SpGEMM forward with respect to the edge
values, held bit for bit to the numpy restatement of its summation tree
(test_edge_grad_capi.edge_grad_rows; include/maxk_hip.h "Edge-value gradient"): where the
restatement gives a NaN the kernel gives a NaN, everywhere else the bits are equal, nothing is
excluded. Then the output contract on poisoned, guarded buffers, and the autograd, layer and
torch-operator surfaces built on the kernel."""
import numpy as np
import pytest
import torch

import maxk_kernels as mk
from arena import POISONS, arena
from maxk_kernels import _lib, ops
from test_edge_grad_capi import edge_grad_rows, gamma

pytestmark = pytest.mark.gpu

CHUNK = 1024   # CSR edges per work-group of the kernel (csrc/sddmm.hip)


# ------------------------------------------------------------------ inputs
def _csr(deg, cols, rng=None):
    """ptr / idx (numpy) from per-row degrees; ``cols``: an idx array, or the number of columns
    to draw from."""
    deg = np.asarray(deg, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    e = int(ptr[-1])
    idx = (np.asarray(cols) if not np.isscalar(cols) else rng.integers(0, cols, e)).astype(np.int32)
    assert idx.size == e
    return ptr, idx


def graph_cases():
    """name -> (ptr, idx, num_cols): the smallest shapes at which the chunk and row logic of the
    kernel can go wrong."""
    rng = np.random.default_rng(10)
    g = {}
    g["one"] = _csr([1], [0]) + (1,)
    # empty rows at the start, in the middle (1200 of them inside one chunk) and at the end
    deg = np.zeros(1500, dtype=np.int64)
    deg[100:130] = rng.integers(1, 40, 30)
    deg[1330:1400] = rng.integers(0, 60, 70)
    g["empty_rows"] = _csr(deg, 200, rng) + (200,)
    # all edges in one row, more than four chunks of it
    g["hub_row"] = _csr([0, 4 * CHUNK + 77, 0], 300, rng) + (300,)
    deg = rng.integers(0, 120, 50)
    g["one_column"] = _csr(deg, np.full(deg.sum(), 7)) + (9,)
    # rows that straddle every chunk boundary
    g["straddle"] = _csr([CHUNK - 1, CHUNK, CHUNK + 1, CHUNK - 1, CHUNK + 1, CHUNK, 5], 500,
                         rng) + (500,)
    # as many rows as edges inside a chunk (far more than a staged batch of rows would hold)
    g["degree_one"] = _csr(np.ones(2000, dtype=np.int64), 700, rng) + (700,)
    deg = rng.integers(0, 30, 120)
    idx = np.sort(rng.integers(0, 6, deg.sum()))   # 6 columns: most (r, c) pairs repeat
    g["duplicate_edges"] = _csr(deg, idx) + (6,)
    g["rect_wide"] = _csr(rng.integers(0, 50, 90), 1900, rng) + (1900,)
    g["rect_tall"] = _csr(rng.integers(0, 8, 1700), 40, rng) + (40,)
    return g


GRAPHS = graph_cases()
MIXED = _csr(np.concatenate([np.random.default_rng(11).integers(0, 40, 250), [CHUNK + 3, 0, 0, 1]]),
             180, np.random.default_rng(12)) + (180,)


def tables(nc, k, d, rng, values="normal", repeat=False, padding=False):
    if values == "ints":
        v = rng.integers(-4, 5, (nc, k)).astype(np.float32)
    elif values == "wide":
        v = (rng.choice([-1.0, 1.0], (nc, k)) * np.exp2(rng.uniform(-60, 60, (nc, k)))
             ).astype(np.float32)
    else:
        v = rng.standard_normal((nc, k)).astype(np.float32)
    if repeat:
        ix = rng.integers(0, min(d, max(2, k // 2)), (nc, k)).astype(np.uint8)
    else:   # ascending distinct selectors, as the top-k emits them
        ix = np.sort(np.argsort(rng.random((nc, d)), axis=1)[:, :k], axis=1).astype(np.uint8)
    if padding:   # ref_compat rows: the slots past count are (0.0f, 0)
        count = rng.integers(0, k + 1, nc)
        pad = np.arange(k)[None, :] >= count[:, None]
        v[pad], ix[pad] = 0.0, 0
    return v, ix


def grads(n, d, rng, values="normal"):
    if values == "ints":
        return rng.integers(-3, 4, (n, d)).astype(np.float32)
    if values == "wide":
        return (rng.choice([-1.0, 1.0], (n, d)) * np.exp2(rng.uniform(-60, 60, (n, d)))
                ).astype(np.float32)
    return rng.standard_normal((n, d)).astype(np.float32)


def _shifted(a, dev):
    """``a`` on the device one element into its buffer: element-aligned only."""
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device=dev)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _row_strided(a, stride, dev):
    buf = torch.zeros((a.shape[0], stride), dtype=torch.from_numpy(a).dtype, device=dev)
    view = buf[:, :a.shape[1]]
    view.copy_(torch.from_numpy(a))
    return view


def run(dev, ptr, idx, G, v, ix, layout="plain"):
    """The kernel's grad_val (numpy) for numpy inputs, the tables laid out as ``layout``."""
    n, d = G.shape
    nc, k = v.shape
    tp, ti = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
    tg, tv, tx = (torch.from_numpy(G).to(dev), torch.from_numpy(v).to(dev),
                  torch.from_numpy(ix).to(dev))
    if layout == "records":   # interleaved layout-1 records, read in place
        rec = torch.zeros((nc, (5 * k + 15) // 16 * 16 + 16), dtype=torch.uint8, device=dev)
        rv, rx = rec[:, :4 * k].view(torch.float32), rec[:, 4 * k:5 * k]
        rv.copy_(tv)
        rx.copy_(tx)
        tv, tx = rv, rx
    elif layout == "unaligned":
        tg, tv, tx = _shifted(G, dev), _shifted(v, dev), _shifted(ix, dev)
    elif layout == "grad_stride":
        tg = _row_strided(G, d + 4, dev)
    elif layout == "table_strides":
        tv, tx = _row_strided(v, k + 3, dev), _row_strided(ix, k + 5, dev)
    else:
        assert layout == "plain"
    out = ops.spgemm_edge_grad(tp, ti, tg, tv, tx, n, idx.size, k, d)
    assert out.shape == (idx.size,) and out.dtype == torch.float32
    return out.cpu().numpy()


def assert_same_bits(got, want, what=""):
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.flatnonzero(gn != wn)[:5]}"
    gb, wb = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} edges differ, first "
                           f"{got[~gn][bad[:3]]} vs {want[~wn][bad[:3]]}")


def check(dev, graph, k, d, seed, values="normal", layout="plain", **tab):
    ptr, idx, nc = graph
    rng = np.random.default_rng(seed)
    n = ptr.size - 1
    v, ix = tables(nc, k, d, rng, values=values, **tab)
    G = grads(n, d, rng, values=values)
    got = run(dev, ptr, idx, G, v, ix, layout)
    assert_same_bits(got, edge_grad_rows(ptr, idx, G, v, ix), f"k={k} D={d} {values} {layout}")
    return got


# ------------------------------------------------------------------ kernel against restatement
@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_graph_shapes(gpu, name, k):
    got = check(gpu, GRAPHS[name], k, 64, seed=k)
    assert got.size == GRAPHS[name][1].size


@pytest.mark.parametrize("k,d", [(k, d) for d in (64, 256) for k in (1, 2, 3, 8, 16, 24, 32, 64)] +
                         [(4, 4), (256, 256)])
def test_k_and_d(gpu, k, d):
    check(gpu, MIXED, k, d, seed=100 + k + d)
    check(gpu, GRAPHS["degree_one"], k, d, seed=200 + k + d, values="ints")


@pytest.mark.parametrize("k", [3, 16, 24])
@pytest.mark.parametrize("layout", ["records", "unaligned", "grad_stride", "table_strides"])
def test_table_layouts(gpu, layout, k):
    if layout == "records" and k % 4:
        k = 32          # records of layout 1 exist at k % 4 == 0 only
    check(gpu, MIXED, k, 64, seed=300 + k, layout=layout)
    check(gpu, GRAPHS["straddle"], k, 256, seed=301 + k, layout=layout)


@pytest.mark.parametrize("k,d", [(3, 64), (16, 64), (24, 256)])
def test_repeated_selectors_and_padding_slots(gpu, k, d):
    check(gpu, MIXED, k, d, seed=400 + k, repeat=True)
    check(gpu, MIXED, k, d, seed=401 + k, padding=True)
    check(gpu, MIXED, k, d, seed=402 + k, values="ints", repeat=True, padding=True)


@pytest.mark.parametrize("k,d", [(2, 64), (3, 64), (8, 64), (16, 256), (24, 64), (64, 256)])
@pytest.mark.parametrize("values", ["ints", "wide"])
def test_exact_and_wide_range_values(gpu, values, k, d):
    check(gpu, MIXED, k, d, seed=500 + k, values=values)


@pytest.mark.parametrize("k,d", [(1, 64), (3, 64), (16, 64), (24, 256)])
def test_non_finite_values(gpu, k, d):
    ptr, idx, nc = MIXED
    rng = np.random.default_rng(600 + k)
    n = ptr.size - 1
    v, ix = tables(nc, k, d, rng)
    G = grads(n, d, rng)
    for a in (v, G):
        flat = a.reshape(-1)
        pos = rng.choice(flat.size, 12, replace=False)
        flat[pos] = np.array([np.inf, -np.inf, np.nan, 0.0] * 3, dtype=np.float32)
    want = edge_grad_rows(ptr, idx, G, v, ix)
    assert np.isnan(want).any() and np.isinf(want).any()
    assert_same_bits(run(gpu, ptr, idx, G, v, ix), want, f"non-finite k={k}")


# ------------------------------------------------------------------ output contract
def _raw(dev, ptr, idx, G, v, ix, out_ptr, n=None, e=None):
    n = G.shape[0] if n is None else n
    e = idx.numel() if e is None else e
    rc = _lib.lib.maxk_sddmm_edge_grad(ptr.data_ptr(), idx.data_ptr(), G.data_ptr(), 0,
                                       v.data_ptr(), 0, ix.data_ptr(), 0, out_ptr, n, v.shape[0],
                                       e, G.shape[1], v.shape[1],
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib.maxk_last_error()


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name,k", [("straddle", 16), ("degree_one", 3), ("hub_row", 32),
                                    ("one", 1)])
def test_grad_val_is_fully_overwritten_and_nothing_else(gpu, name, k, poison):
    ptr, idx, nc = GRAPHS[name]
    rng = np.random.default_rng(700 + k)
    n, d = ptr.size - 1, 64
    v, ix = tables(nc, k, d, rng)
    G = grads(n, d, rng)
    t = [torch.from_numpy(a).to(gpu) for a in (ptr, idx, G, v, ix)]
    a = arena((1, idx.size, torch.float32), gpu, poison)
    _raw(gpu, *t, a.ptr)
    torch.cuda.synchronize()
    assert a.check() is None, a.check()
    assert a.first_poisoned() is None, a.first_poisoned()
    want = edge_grad_rows(ptr, idx, G, v, ix)
    assert_same_bits(a.payload[0].cpu().numpy(), want, name)
    b = arena((1, idx.size, torch.float32), gpu, poison)     # two runs: identical bits
    _raw(gpu, *t, b.ptr)
    assert torch.equal(a.payload.view(torch.int32), b.payload.view(torch.int32))


@pytest.mark.parametrize("poison", POISONS)
def test_empty_calls_write_nothing(gpu, poison):
    ptr, idx, nc = MIXED
    rng = np.random.default_rng(8)
    v, ix = tables(nc, 16, 64, rng)
    G = grads(ptr.size - 1, 64, rng)
    t = [torch.from_numpy(a).to(gpu) for a in (ptr, idx, G, v, ix)]
    a = arena(4096, gpu, poison)
    _raw(gpu, *t, a.ptr, e=0)
    _raw(gpu, *t, a.ptr, n=0)
    _raw(gpu, *t, a.ptr, n=0, e=0)
    torch.cuda.synchronize()
    assert a.check() is None
    assert bool((a.payload == poison).all())


# ------------------------------------------------------------------ autograd
# The SSpMM backward adds a column's terms into f32 LDS accumulators in the order its waves
# arrive, so x.grad is the same from run to run (and between the weighted and the baked call)
# only where every f32 sum is exact. The bit-for-bit comparisons therefore run on edge values,
# edge weights and upstream gradients that are small dyadic numbers: every product and partial
# sum is exact in any order (below 2^18 in units of 2^-4, see _exact_weights), and a wrong
# index, a stale value snapshot or a missed refresh still changes bits. x itself is random
# normal: it enters the forward (fixed point, order-free) and the edge gradient, whose order the
# kernel fixes.
N_AG, E_AG, D_AG, K_AG = 300, 3000, 64, 16


def _pick(dev, shape, choices, seed):
    gen = torch.Generator().manual_seed(seed)
    c = torch.tensor(choices, dtype=torch.float32)
    return c[torch.randint(len(choices), shape, generator=gen)].to(dev)


def _exact_weights(dev, e, seed):
    """Edge weights in {0.5, 1, 1.5} on base values in {0.5, 1, 2}: effective values are
    multiples of 2^-2 up to 3. With upstream gradients in {-2 .. 2} a column's sum over its
    at most 2^6 in-edges is a multiple of 2^-2 below 2^9, and one layer further down a multiple
    of 2^-4 below 2^17: 21 bits, exact in f32 in any order."""
    return _pick(dev, (e,), [0.5, 1.0, 1.5], seed)


def _exact_grads(dev, shape, seed):
    return _pick(dev, shape, [-2.0, -1.0, 0.0, 1.0, 2.0], seed)


def _ag_graph(dev, seed=21):
    from maxk_kernels import graphs
    ptr, idx = graphs.synthetic_csr(N_AG, E_AG, seed=seed)
    val = _pick(dev, (idx.numel(),), [0.5, 1.0, 2.0], seed)
    g = mk.CSRGraph(ptr.to(dev), idx.to(dev), val)
    assert int(g.out_degrees().max()) <= 64   # terms of one SSpMM sum (_exact_weights)
    return g


def _randn(dev, shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _weights(dev, e, seed):
    return (torch.rand(e, generator=torch.Generator().manual_seed(seed)) + 0.5).to(dev)


def _call(form, x, g, mode, p, ew):
    """One of the three entry points -> (outputs, the CBSR tables its aggregation consumed)."""
    kw = dict(dropout_p=p, training=True, seed=77)
    if form == "spgemm":
        sp_data, sp_index = mk.maxk(x, K_AG, mode, **kw)
        return (mk.spgemm(sp_data, sp_index, g, D_AG, edge_weight=ew),)
    if form == "aggregate":
        return (mk.maxk_aggregate(x, g, K_AG, mode, edge_weight=ew, **kw),)
    return tuple(mk.maxk_self_aggregate(x, g, K_AG, mode, edge_weight=ew, **kw))


def _tables(x, mode, p):
    v, ix = ops.maxk_forward(x.detach(), K_AG, mode=mode, return_index=True,
                             dropout=(p, 77) if p else None)
    return v.cpu().numpy(), ix.cpu().numpy()


def _edge_weight_grad_checks(g, gout, v, ix, ew_grad, what):
    """ew.grad is base_val * edge_grad_rows bit for bit, and within the gamma bound of the
    float64 composition: k + 1 roundings on the way to grad_val's restated sum (test_edge_grad_
    capi) and one more for the multiply by the base value, so gamma(k + 2) * val * sum |x g|."""
    ptr, idx, val = g.ptr.cpu().numpy(), g.idx.cpu().numpy(), g.val.cpu().numpy()
    G = gout.cpu().numpy()
    want = (val * edge_grad_rows(ptr, idx, G, v, ix)).astype(np.float32)
    assert_same_bits(ew_grad.cpu().numpy(), want, what)
    rows = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    prod = v[idx].astype(np.float64) * G[rows[:, None], ix[idx].astype(np.int64)].astype(np.float64)
    exact = val.astype(np.float64) * prod.sum(1)
    bound = gamma(K_AG + 2) * val.astype(np.float64) * np.abs(prod).sum(1)
    assert np.all(np.abs(ew_grad.cpu().numpy().astype(np.float64) - exact) <= bound), what


@pytest.mark.parametrize("mode", ["exact", "ref_compat"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("form", ["spgemm", "aggregate", "self"])
def test_autograd_with_edge_weight(gpu, form, p, mode):
    g = _ag_graph(gpu)
    x0 = _randn(gpu, (N_AG, D_AG), 1)
    gouts = [_exact_grads(gpu, (N_AG, D_AG), 2 + i) for i in range(2 if form == "self" else 1)]
    ew = _exact_weights(gpu, g.num_edges, 3).requires_grad_(True)
    x = x0.clone().requires_grad_(True)
    outs = _call(form, x, g, mode, p, ew)
    torch.autograd.backward(outs, gouts)
    # the same call with the effective values baked into graph.val and no edge_weight
    baked = mk.CSRGraph(g.ptr, g.idx, (g.val * ew).detach())
    xb = x0.clone().requires_grad_(True)
    outs_b = _call(form, xb, baked, mode, p, None)
    torch.autograd.backward(outs_b, gouts)
    for a, b in zip(outs, outs_b):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(x.grad.view(torch.int32), xb.grad.view(torch.int32))
    v, ix = _tables(x0, mode, p)
    _edge_weight_grad_checks(g, gouts[-1], v, ix, ew.grad, f"{form} p={p} {mode}")


@pytest.mark.parametrize("form", ["spgemm", "aggregate", "self"])
def test_without_edge_weight_nothing_changes(gpu, form):
    g = _ag_graph(gpu)
    x0 = _randn(gpu, (N_AG, D_AG), 1)
    res = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        outs = _call(form, x, g, "exact", 0.5, None)
        torch.autograd.backward(outs, [_exact_grads(gpu, (N_AG, D_AG), 5)] * len(outs))
        res.append([o.detach() for o in outs] + [x.grad])
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not any(isinstance(k, tuple) and k[0] == "weighted_plan" for k in g._values)


def test_constant_values_save_no_value_table(gpu):
    """edge_weight without requires_grad: the result is the baked one and the backward gets
    no value table (nothing new is saved on the path that needs no val gradient)."""
    g = _ag_graph(gpu)
    x = _randn(gpu, (N_AG, D_AG), 1).requires_grad_(True)
    y = mk.maxk_aggregate(x, g, K_AG, edge_weight=_weights(gpu, g.num_edges, 3))
    assert len(y.grad_fn.saved_tensors) == 1 and y.grad_fn.saved_tensors[0].dtype == torch.uint8
    y.backward(torch.ones_like(y))
    assert x.grad is not None


def test_two_stacked_layers_share_one_plan(gpu):
    """Layer 1's backward runs after layer 2's forward left its own values in the shared
    weighted plan: the re-refresh rule."""
    g = _ag_graph(gpu)
    x0 = _randn(gpu, (N_AG, D_AG), 1)
    gout = _exact_grads(gpu, (N_AG, D_AG), 2)
    ew1 = _exact_weights(gpu, g.num_edges, 3).requires_grad_(True)
    ew2 = _exact_weights(gpu, g.num_edges, 4).requires_grad_(True)
    x = x0.clone().requires_grad_(True)
    h = mk.maxk_aggregate(x, g, K_AG, edge_weight=ew1)
    h.retain_grad()
    y = mk.maxk_aggregate(h, g, K_AG, edge_weight=ew2)
    assert g.weighted_plan(D_AG, K_AG)._refs[2] is not None
    y.backward(gout)
    g1 = mk.CSRGraph(g.ptr, g.idx, (g.val * ew1).detach())
    g2 = mk.CSRGraph(g.ptr, g.idx, (g.val * ew2).detach())
    xb = x0.clone().requires_grad_(True)
    hb = mk.maxk_aggregate(xb, g1, K_AG)
    yb = mk.maxk_aggregate(hb, g2, K_AG)
    yb.backward(gout)
    assert torch.equal(y.view(torch.int32), yb.view(torch.int32))
    assert torch.equal(x.grad.view(torch.int32), xb.grad.view(torch.int32))
    v, ix = _tables(h, "exact", 0.0)
    _edge_weight_grad_checks(g, gout, v, ix, ew2.grad, "second layer")
    v, ix = _tables(x0, "exact", 0.0)
    _edge_weight_grad_checks(g, h.grad, v, ix, ew1.grad, "first layer")


def test_fresh_weights_every_step_build_no_plan(gpu):
    g = _ag_graph(gpu)
    x = _randn(gpu, (N_AG, D_AG), 1).requires_grad_(True)
    plans, handles, cached = [], [], []
    for step in range(3):
        ew = _weights(gpu, g.num_edges, 10 + step).requires_grad_(True)
        mk.maxk_aggregate(x, g, K_AG, edge_weight=ew).sum().backward()
        assert ew.grad is not None
        plans.append(g.weighted_plan(D_AG, K_AG))
        handles.append(plans[-1].handle.value)
        cached.append(ops.cached_plan_bytes())
    assert plans[0] is plans[1] is plans[2] and len(set(handles)) == 1
    assert len(set(cached)) == 1
    assert sum(isinstance(k, tuple) and k[0] == "weighted_plan" for k in g._values) == 1


# ------------------------------------------------------------------ layers
def _dense_adjacency(csr, ew):
    """float64 [N, N] of the effective values (duplicate edges sum), and the row of each edge."""
    n = csr.num_nodes
    rows = torch.repeat_interleave(torch.arange(n, device=csr.device), csr.in_degrees())
    a = torch.zeros((n, n), dtype=torch.float64, device=csr.device)
    a.index_put_((rows, csr.idx.long()), csr.val.double() * ew.double(), accumulate=True)
    return a, rows


def _topk_mask(x, k):
    return torch.zeros_like(x).scatter_(1, x.topk(k, dim=1).indices, 1.0)


@pytest.mark.parametrize("nonlinear", ["maxk", "relu"])
@pytest.mark.parametrize("kind", ["gcn", "sage", "gin"])
def test_layers_with_edge_weight_match_the_dgl_formulas(gpu, kind, nonlinear):
    """Against a dense float64 restatement of DGL's layer with ``edge_weight`` (normalisation
    from the unweighted degrees, message u_mul_e). With u = 2^-24, gamma(n) = n u / (1 - n u)
    bounds any f32 evaluation of an n-term sum of products. x is what the layer aggregates
    (MaxK(feat), or feat for relu), exactly representable in both computations.

    * agg = A_eff x: val * ew is one rounding, each term one more, a row has at most maxdeg
      terms and the result one final rounding: |err agg| <= E_agg = gamma(maxdeg + 3) |A_eff| |x|.
    * GCN: out = agg + b, one more add: E_agg + 2u |out|. GIN: out = (1 + eps) x + agg, three
      more operations: E_agg + gamma(3) (|(1 + eps) x| + |agg|).
    * SAGE: out = x Ws^T + agg Wn^T + b: two f32 GEMMs with inner size D and two adds,
      gamma(D + 3) (|x| |Ws|^T + |agg| |Wn|^T + |b|), plus the aggregation's error carried
      through the GEMM, E_agg |Wn|^T (times 1 + gamma(D + 3)).
    * edge_weight.grad[e] = val[e] * sum_f Gagg[r, f] x[c, f] with K terms (k, or D for relu):
      gamma(K + 2) val sum |Gagg| |x| for the kernel's products, tree and the multiply by val;
      Gagg is the incoming gradient itself (GCN, GIN) or gout Wn, an f32 GEMM with inner size
      D and error E_G = gamma(D) |gout| |Wn|, which enters as val sum E_G |x| (1 + gamma(K + 2))."""
    torch.manual_seed(0)
    n, d, k = N_AG, D_AG, K_AG
    g = _ag_graph(gpu)
    feat = _randn(gpu, (n, d), 31)
    gout = _randn(gpu, (n, d), 32)
    ew = _weights(gpu, g.num_edges, 33).requires_grad_(True)
    if kind == "gcn":
        layer, norm = mk.MaxKGCNConv(d, d, norm="both", weight=False, maxk=k,
                                     allow_zero_in_degree=True, nonlinear=nonlinear), "both"
    elif kind == "sage":
        layer, norm = mk.MaxKSAGEConv(d, d, "mean", maxk=k, nonlinear=nonlinear), "mean"
    else:
        layer, norm = mk.MaxKGINConv(d, maxk=k, init_eps=0.25, nonlinear=nonlinear), "sum"
    layer = layer.to(gpu)
    if getattr(layer, "bias", None) is not None:
        with torch.no_grad():
            layer.bias.copy_(_randn(gpu, (d,), 34))
    out = layer(g, feat, edge_weight=ew)
    out.backward(gout)

    csr = g.with_values(norm)
    ew64 = ew.detach().double().requires_grad_(True)
    a, rows = _dense_adjacency(csr, ew64)
    x = (feat * _topk_mask(feat, k) if nonlinear == "maxk" else feat).double()
    agg = a @ x
    maxdeg = int(g.in_degrees().max())
    K = k if nonlinear == "maxk" else d
    e_agg = gamma(maxdeg + 3) * (a.detach().abs() @ x.abs())
    g64 = gout.double()
    if kind == "gcn":
        ref = agg + layer.bias.detach().double()
        tol = e_agg + 2 * 2.0 ** -24 * ref.detach().abs()
        gagg, e_g = g64, torch.zeros_like(g64)
    elif kind == "gin":
        eps = layer.eps.detach().double()
        ref = (1 + eps) * x + agg
        tol = e_agg + gamma(3) * (((1 + eps) * x).abs() + agg.detach().abs())
        gagg, e_g = g64, torch.zeros_like(g64)
    else:
        ws, wn = layer.fc_self.weight.detach().double(), layer.fc_neigh.weight.detach().double()
        b = layer.bias.detach().double()
        ref = x @ ws.T + agg @ wn.T + b
        tol = (gamma(d + 3) * (x.abs() @ ws.abs().T + agg.detach().abs() @ wn.abs().T + b.abs()) +
               (1 + gamma(d + 3)) * (e_agg @ wn.abs().T))
        gagg, e_g = g64 @ wn, gamma(d) * (g64.abs() @ wn.abs())
    assert bool(((out.detach().double() - ref.detach()).abs() <= tol).all()), \
        float(((out.detach().double() - ref.detach()).abs() - tol).max())
    ref.backward(g64)
    cols = csr.idx.long()
    mag = (gagg.abs()[rows] * x.abs()[cols]).sum(1)
    gbound = csr.val.double() * ((1 + gamma(K + 2)) * (e_g[rows] * x.abs()[cols]).sum(1) +
                                 gamma(K + 2) * mag)
    err = (ew.grad.double() - ew64.grad).abs()
    assert bool((err <= gbound).all()), float((err - gbound).max())
    assert float(ew.grad.abs().sum()) > 0


def test_models_pass_edge_weight_through(gpu):
    g = _ag_graph(gpu)
    x = _randn(gpu, (N_AG, 32), 41)
    for cls in (mk.MaxKSAGE, mk.MaxKGCN, mk.MaxKGIN):
        torch.manual_seed(1)
        model = cls(32, D_AG, 2, 8, maxk=K_AG, feat_drop=0.0).to(gpu)
        ew = _weights(gpu, g.num_edges, 42).requires_grad_(True)
        y = model(g, x, edge_weight=ew)
        y.square().sum().backward()
        assert ew.grad is not None and float(ew.grad.abs().sum()) > 0
        ones = torch.ones(g.num_edges, device=gpu)
        torch.testing.assert_close(model(g, x, edge_weight=ones), model(g, x), atol=1e-5, rtol=1e-5)


def test_dgl_graph_with_edge_weight_is_a_type_error(gpu):
    class DGLLike:
        def adj_tensors(self, fmt):
            raise AssertionError("not reached")

    ew = torch.ones(4, device=gpu)
    x = torch.zeros(4, D_AG, device=gpu)
    for layer in (mk.MaxKGCNConv(D_AG, D_AG, weight=False, maxk=K_AG), mk.MaxKGINConv(D_AG, maxk=K_AG),
                  mk.MaxKSAGEConv(D_AG, D_AG, maxk=K_AG)):
        with pytest.raises(TypeError, match="CSRGraph"):
            layer.to(gpu)(DGLLike(), x, edge_weight=ew)


# ------------------------------------------------------------------ torch operator
def test_edge_grad_operator_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        ptr = torch.empty(51, dtype=torch.int32, device="cuda")
        idx = torch.empty(300, dtype=torch.int32, device="cuda")
        gout = torch.empty(50, 64, device="cuda")
        v = torch.empty(50, 16, device="cuda")
        ix = torch.empty(50, 16, dtype=torch.uint8, device="cuda")
        gv = torch.ops.maxk.spgemm_edge_grad(ptr, idx, gout, v, ix, 50, 300, 16, 64)
        assert gv.shape == (300,) and gv.dtype == torch.float32 and gv.device.type == "cuda"


def test_edge_grad_operator_compiles_and_differentiates(gpu):
    g = _ag_graph(gpu)
    x = _randn(gpu, (N_AG, D_AG), 51)
    gout = _randn(gpu, (N_AG, D_AG), 52)
    v, ix = mk.maxk_forward(x, K_AG, return_index=True)
    args = (g.ptr, g.idx, gout, v, ix, N_AG, g.num_edges, K_AG, D_AG)
    want = edge_grad_rows(g.ptr.cpu().numpy(), g.idx.cpu().numpy(), gout.cpu().numpy(),
                          v.cpu().numpy(), ix.cpu().numpy())
    torch.library.opcheck(torch.ops.maxk.spgemm_edge_grad.default, args)
    seen = []

    def backend(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == "call_function")
        return gm.forward

    fn = torch.compile(lambda *a: torch.ops.maxk.spgemm_edge_grad(*a) * 1.0, backend=backend,
                       fullgraph=True)
    assert_same_bits(fn(*args).cpu().numpy(), want, "compiled")
    assert any("spgemm_edge_grad" in t for t in seen), seen
    # the registered derivative of spgemm_forward returns it for a val that requires grad
    val = g.val.clone().requires_grad_(True)
    y = torch.ops.maxk.spgemm_forward(g.ptr, g.idx, val, v, ix, N_AG, g.num_edges, K_AG, D_AG)
    y.backward(gout)
    assert_same_bits(val.grad.cpu().numpy(), want, "spgemm_forward val gradient")
