"""GPU: maxk_gat_attention_forward / _backward and maxk_edge_colsum against the composition they
fuse (bit for bit where include/maxk_hip.h, "GAT attention", says so, within the derived sum
bounds elsewhere), their output contract, graph capture, the autograd Function, the registered
operators and MaxKGATConv(fused_attention=True).

One graph serves most tests (test_gat_attention_capi.graph_arrays): row lengths and column
lengths both run through every regime and both sides of every limit the library reports."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

import maxk_kernels as mk
import test_gpu_edge_softmax as tges
from arena import POISONS, arena
from maxk_kernels import _lib, attention, ops
from test_gat_attention_capi import (col_sum_bound, col_sums64, graph_arrays, row_sum_bound,
                                     row_sums64, transposed)
from test_gpu_edge_softmax import REGIMES, assert_same_bits, bits, dev_of, ptr_of, regime

pytestmark = pytest.mark.gpu

SLOPES = (0.2, 0.0, 1.0)


def rows_of(ptr):
    return np.repeat(np.arange(ptr.size - 1), np.diff(ptr))


@functools.lru_cache(maxsize=None)
def scores_of(R, seed=3):
    """(el, er) f32 for the test graph with z = el[c] + er[r] in (-R / 2, R / 2), both signs, and
    with a few rows and columns arranged so that scores of exactly +0.0 and -0.0 occur."""
    ptr, idx = graph_arrays()
    n = ptr.size - 1
    rng = np.random.default_rng(seed)
    el = (rng.random(n) * R / 2).astype(np.float32)
    er = (-rng.random(n) * R / 2).astype(np.float32)
    rows = rows_of(ptr)
    hub = int(np.diff(ptr).argmax())
    er[hub] = -0.0
    cols = idx[rows == hub]
    el[cols[::7]] = 0.0           # +0.0 + -0.0 = +0.0
    el[cols[3::7]] = -0.0         # -0.0 + -0.0 = -0.0
    z = el[idx] + er[rows]
    assert ((bits(z) == 0).any() and (bits(z) == 0x80000000).any() and (z > 0).any() and
            (z < 0).any())
    for a in (el, er):
        a.setflags(write=False)
    return el, er


def graph_dev(dev):
    ptr, idx = graph_arrays()
    return dev_of(ptr, dev), dev_of(idx, dev), dev_of(rows_of(ptr), dev)


def composition(ptr, idx, rows, el, er, slope):
    """What the fused forward replaces: torch's gather, add and leaky-relu, then the softmax."""
    return ops.edge_softmax(ptr, F.leaky_relu(el[idx.long()] + er[rows], slope))


def grad_edge_composition(ptr, idx, rows, el, er, slope, alpha, g):
    z = el[idx.long()] + er[rows]
    return torch.ops.aten.leaky_relu_backward(ops.edge_softmax_backward(ptr, alpha, g), z, slope,
                                              False)


def worst_by_length(err, bound, lengths, what):
    """Prints the worst error / bound per regime (pytest -s) and asserts it is <= 1; where the
    bound is 0 (an empty segment, or all-zero terms) the error must be 0."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    reg = np.array([regime(int(n)) for n in lengths])
    worst = [float(ratio[reg == r].max(initial=0.0)) for r in range(REGIMES)]
    print(f"\n{what}: worst error / bound per regime {['%.3f' % w for w in worst]}")
    assert np.isfinite(ratio).all() and max(worst) <= 1.0, (what, worst)


def gvec(dev, seed, n=None):
    n = graph_arrays()[1].size if n is None else n
    return dev_of(np.random.default_rng(seed).standard_normal(n).astype(np.float32), dev)


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("R", [0.5, 60.0])
@pytest.mark.parametrize("slope", SLOPES)
def test_forward_is_the_softmax_of_the_materialised_scores_bit_for_bit(gpu, slope, R):
    ptr, idx, rows = graph_dev(gpu)
    el, er = (dev_of(a, gpu) for a in scores_of(R))
    got = ops.gat_attention(ptr, idx, el, er, slope)
    assert got.dtype == torch.float32 and got.shape == idx.shape
    want = composition(ptr, idx, rows, el, er, slope)
    assert_same_bits(got.cpu().numpy(), want.cpu().numpy(), f"slope={slope} R={R}")
    sums = row_sums64(graph_arrays()[0], got.cpu().numpy())
    assert np.all(np.abs(sums[np.diff(graph_arrays()[0]) > 0] - 1) < 1e-4)


def test_forward_non_finite_scores(gpu):
    """-Inf in el: +0.0f on that column's edges wherever the row holds a finite score. NaN or
    +Inf in er[r]: exactly row r is NaN. NaN in el[c]: exactly the rows holding column c."""
    ptr_np, idx_np = graph_arrays()
    rows_np = rows_of(ptr_np)
    ptr, idx, rows = graph_dev(gpu)
    el_np, er_np = scores_of(0.5)
    clean = ops.gat_attention(ptr, idx, dev_of(el_np, gpu), dev_of(er_np, gpu), 0.2).cpu().numpy()
    deg = np.diff(ptr_np)
    c = int(np.flatnonzero(np.bincount(idx_np, minlength=deg.size) == 65)[0])

    def run(el, er):
        el, er = dev_of(el, gpu), dev_of(er, gpu)
        got = ops.gat_attention(ptr, idx, el, er, 0.2)
        want = composition(ptr, idx, rows, el, er, 0.2)
        got, want = got.cpu().numpy(), want.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert_same_bits(got[~np.isnan(got)], want[~np.isnan(want)], "non-finite, composition")
        return got

    el = el_np.copy()
    el[c] = -np.inf
    got = run(el, er_np)
    on_c = idx_np == c
    finite_row = np.zeros(deg.size, bool)
    finite_row[rows_np[~on_c]] = True
    sel = on_c & finite_row[rows_np]
    assert sel.sum() >= 32 and np.all(bits(got[sel]) == 0)
    assert np.isnan(got[on_c & ~finite_row[rows_np]]).all() and not np.isnan(got[~on_c]).any()

    for bad in (np.nan, np.inf):
        er = er_np.copy()
        hit = [int(np.flatnonzero(deg == n)[0]) for n in (3, 128, int(deg.max()))]
        er[hit] = bad
        got = run(el_np, er)
        in_hit = np.isin(rows_np, hit)
        assert np.isnan(got[in_hit]).all()
        assert_same_bits(got[~in_hit], clean[~in_hit], "rows beside a non-finite er")

    el = el_np.copy()
    el[c] = np.nan
    got = run(el, er_np)
    in_hit = np.isin(rows_np, np.unique(rows_np[on_c]))
    assert np.isnan(got[in_hit]).all() and 0 < in_hit.sum() < in_hit.size
    assert_same_bits(got[~in_hit], clean[~in_hit], "rows beside a NaN el")


# ------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def backward_of(slope, R=0.5):
    """One backward on the test graph, shared: (alpha, g, grad_edge, grad_er, the composition's
    grad_edge) as numpy."""
    dev = torch.device("cuda:0")
    ptr, idx, rows = graph_dev(dev)
    el, er = (dev_of(a, dev) for a in scores_of(R))
    alpha = ops.gat_attention(ptr, idx, el, er, slope)
    g = gvec(dev, 6)
    grad_edge, grad_er = ops.gat_attention_backward(ptr, idx, el, er, slope, alpha, g)
    want = grad_edge_composition(ptr, idx, rows, el, er, slope, alpha, g)
    out = tuple(t.cpu().numpy() for t in (alpha, g, grad_edge, grad_er, want))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("slope", SLOPES)
def test_grad_edge_is_the_softmax_backward_through_leaky_relu_bit_for_bit(gpu, slope):
    _, _, grad_edge, _, want = backward_of(slope)
    assert_same_bits(grad_edge, want, f"grad_edge slope={slope}")
    assert float(np.abs(grad_edge).sum()) > 0


@pytest.mark.parametrize("slope", SLOPES)
def test_grad_er_is_the_row_sum_within_its_bound(gpu, slope):
    ptr = graph_arrays()[0]
    _, _, grad_edge, grad_er, _ = backward_of(slope)
    assert grad_er.dtype == np.float32 and grad_er.shape == (ptr.size - 1,)
    worst_by_length(np.abs(grad_er.astype(np.float64) - row_sums64(ptr, grad_edge)),
                    row_sum_bound(ptr, grad_edge), np.diff(ptr), f"grad_er slope={slope}")
    empty = np.diff(ptr) == 0
    assert empty.sum() >= 4 and np.all(bits(grad_er[empty]) == 0)


# ------------------------------------------------------------------ column sum
def test_colsum_exact_values_bit_for_bit(gpu):
    ptr, idx = graph_arrays()
    n = ptr.size - 1
    pt, order = transposed(idx, n)
    v = (np.random.default_rng(7).integers(-8, 9, idx.size) * 0.5).astype(np.float32)
    got = ops.edge_colsum(dev_of(pt, gpu), dev_of(order, gpu), dev_of(v, gpu)).cpu().numpy()
    want = col_sums64(idx, v, n).astype(np.float32)
    assert_same_bits(got, want, "exactly summable values")
    empty = np.bincount(idx, minlength=n) == 0
    assert empty.sum() >= 4 and np.all(bits(got[empty]) == 0)
    # the graph's own transposed structure is the same one
    g = mk.CSRGraph(dev_of(ptr, gpu), dev_of(idx, gpu))
    got2 = ops.edge_colsum(g.transposed_structure()[0], g.transposed_order(), dev_of(v, gpu))
    assert_same_bits(got2.cpu().numpy(), want, "CSRGraph.transposed_order")


def test_colsum_random_values_within_the_bound(gpu):
    ptr, idx = graph_arrays()
    n = ptr.size - 1
    pt, order = transposed(idx, n)
    v = np.random.default_rng(8).standard_normal(idx.size).astype(np.float32)
    got = ops.edge_colsum(dev_of(pt, gpu), dev_of(order, gpu), dev_of(v, gpu)).cpu().numpy()
    lengths = np.bincount(idx, minlength=n)
    worst_by_length(np.abs(got.astype(np.float64) - col_sums64(idx, v, n)),
                    col_sum_bound(idx, v, n), lengths, "edge_colsum")
    assert np.all(bits(got[lengths == 0]) == 0)


def test_rectangular_graph(gpu):
    """num_cols != num_rows through ops: forward and grad_edge bit for bit with the composition,
    both sums within their bounds, columns beyond num_rows in use."""
    ptr_np = graph_arrays()[0]
    n, c = ptr_np.size - 1, ptr_np.size - 1 + 37
    rng = np.random.default_rng(9)
    idx_np = rng.integers(0, c, int(ptr_np[-1])).astype(np.int32)
    idx_np[:64] = c - 1
    el_np = (rng.random(c) - 0.5).astype(np.float32)
    er_np = (rng.random(n) - 0.5).astype(np.float32)
    ptr, idx, rows = dev_of(ptr_np, gpu), dev_of(idx_np, gpu), dev_of(rows_of(ptr_np), gpu)
    el, er, g = dev_of(el_np, gpu), dev_of(er_np, gpu), gvec(gpu, 10)
    alpha = ops.gat_attention(ptr, idx, el, er, 0.2)
    assert_same_bits(alpha.cpu().numpy(), composition(ptr, idx, rows, el, er, 0.2).cpu().numpy(),
                     "rectangular forward")
    grad_edge, grad_er = ops.gat_attention_backward(ptr, idx, el, er, 0.2, alpha, g)
    want = grad_edge_composition(ptr, idx, rows, el, er, 0.2, alpha, g)
    assert_same_bits(grad_edge.cpu().numpy(), want.cpu().numpy(), "rectangular grad_edge")
    ge = grad_edge.cpu().numpy()
    worst_by_length(np.abs(grad_er.cpu().numpy().astype(np.float64) - row_sums64(ptr_np, ge)),
                    row_sum_bound(ptr_np, ge), np.diff(ptr_np), "rectangular grad_er")
    pt, order = transposed(idx_np, c)
    grad_el = ops.edge_colsum(dev_of(pt, gpu), dev_of(order, gpu), grad_edge).cpu().numpy()
    assert grad_el.shape == (c,)
    worst_by_length(np.abs(grad_el.astype(np.float64) - col_sums64(idx_np, ge, c)),
                    col_sum_bound(idx_np, ge, c), np.bincount(idx_np, minlength=c),
                    "rectangular grad_el")


# ------------------------------------------------------------------ determinism, position
def test_repeated_calls_are_bitwise_equal(gpu):
    ptr, idx, _ = graph_dev(gpu)
    el, er = (dev_of(a, gpu) for a in scores_of(60.0))
    g = gvec(gpu, 11)
    pt, order = (dev_of(a, gpu) for a in transposed(graph_arrays()[1], ptr.numel() - 1))
    runs = []
    for _ in range(2):
        alpha = ops.gat_attention(ptr, idx, el, er, 0.2)
        ge, ger = ops.gat_attention_backward(ptr, idx, el, er, 0.2, alpha, g)
        runs.append((alpha, ge, ger, ops.edge_colsum(pt, order, ge)))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", [37, 300, 3000])
def test_a_row_and_a_column_give_the_same_bits_wherever_they_sit(gpu, n):
    """One row of fixed contents (its columns' el values, its er, its incoming gradient) at two
    positions of two graphs of different num_rows, and one column of fixed values likewise."""
    rng = np.random.default_rng(n)
    el_row = (rng.random(n) - 0.5).astype(np.float32)
    g_row = rng.standard_normal(n).astype(np.float32)
    er_row = np.float32(0.125)
    seen = []
    for lead, tail in [((5, 0, 70), (2,)), ((1,), (0, 1100, 3, 9))]:
        deg = np.array(lead + (n,) + tail)
        ptr_np, r = ptr_of(deg), len(lead)
        e, c = int(ptr_np[-1]), int(ptr_np[-1]) + 3
        idx_np = rng.integers(0, c, e).astype(np.int32)
        el_np = (rng.random(c) - 0.5).astype(np.float32)
        er_np = (rng.random(deg.size) - 0.5).astype(np.float32)
        g_np = rng.standard_normal(e).astype(np.float32)
        seg = slice(int(ptr_np[r]), int(ptr_np[r + 1]))
        own = rng.permutation(c)[:n].astype(np.int32)        # the row's columns, distinct
        idx_np[seg], el_np[own], er_np[r], g_np[seg] = own, el_row, er_row, g_row
        ptr, idx = dev_of(ptr_np, gpu), dev_of(idx_np, gpu)
        el, er, g = dev_of(el_np, gpu), dev_of(er_np, gpu), dev_of(g_np, gpu)
        alpha = ops.gat_attention(ptr, idx, el, er, 0.2)
        ge, ger = ops.gat_attention_backward(ptr, idx, el, er, 0.2, alpha, g)
        # the same values as one column: column r of a structure whose column lengths are deg
        vals = np.zeros(e, np.float32)
        order_np = rng.permutation(e).astype(np.int32)
        vals[order_np[seg]] = g_row
        col = ops.edge_colsum(ptr, dev_of(order_np, gpu), dev_of(vals, gpu))
        seen.append((alpha[seg].cpu().numpy(), ge[seg].cpu().numpy(),
                     ger[r:r + 1].cpu().numpy(), col[r:r + 1].cpu().numpy()))
    for a, b, what in zip(*seen, ("alpha", "grad_edge", "grad_er", "colsum")):
        assert_same_bits(a, b, f"n={n}: {what}")


# ------------------------------------------------------------------ output contract
def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("poison", POISONS)
def test_outputs_are_fully_overwritten_and_nothing_else(gpu, poison):
    ptr, idx, _ = graph_dev(gpu)
    n, e = ptr.numel() - 1, idx.numel()
    el, er = (dev_of(a, gpu) for a in scores_of(0.5))
    g = gvec(gpu, 12)
    pt, order = (dev_of(a, gpu) for a in transposed(graph_arrays()[1], n))
    ins = (ptr, idx, el, er, g, pt, order)
    keep = [t.clone() for t in ins]
    lib = _lib.lib
    a = arena((1, e, torch.float32), gpu, poison)
    assert lib.maxk_gat_attention_forward(ptr.data_ptr(), idx.data_ptr(), el.data_ptr(),
                                          er.data_ptr(), 0.2, a.ptr, n, n, e, _stream()) == 0
    torch.cuda.synchronize()
    assert a.check() is None and a.first_poisoned() is None
    alpha = a.payload[0].clone()
    assert_same_bits(alpha.cpu().numpy(), ops.gat_attention(ptr, idx, el, er, 0.2).cpu().numpy(),
                     "arena forward")
    b, c = arena((1, e, torch.float32), gpu, poison), arena((1, n, torch.float32), gpu, poison)
    assert lib.maxk_gat_attention_backward(ptr.data_ptr(), idx.data_ptr(), el.data_ptr(),
                                           er.data_ptr(), 0.2, alpha.data_ptr(), g.data_ptr(),
                                           b.ptr, c.ptr, n, n, e, _stream()) == 0
    torch.cuda.synchronize()
    for x in (b, c):
        assert x.check() is None and x.first_poisoned() is None
    ge, ger = ops.gat_attention_backward(ptr, idx, el, er, 0.2, alpha, g)
    assert_same_bits(b.payload[0].cpu().numpy(), ge.cpu().numpy(), "arena grad_edge")
    assert_same_bits(c.payload[0].cpu().numpy(), ger.cpu().numpy(), "arena grad_er")
    d = arena((1, n, torch.float32), gpu, poison)
    assert lib.maxk_edge_colsum(pt.data_ptr(), order.data_ptr(), ge.data_ptr(), d.ptr, n, e,
                                _stream()) == 0
    torch.cuda.synchronize()
    assert d.check() is None and d.first_poisoned() is None
    assert_same_bits(d.payload[0].cpu().numpy(), ops.edge_colsum(pt, order, ge).cpu().numpy(),
                     "arena colsum")
    assert a.check() is None and torch.equal(a.payload[0], alpha)
    for t, k in zip(ins, keep):
        assert torch.equal(t, k)


@pytest.mark.parametrize("poison", POISONS)
def test_calls_without_edges(gpu, poison):
    """E == 0: alpha and grad_edge have no element and nothing of them is written; grad_er and
    out are zero-filled. No rows (columns): nothing at all."""
    lib = _lib.lib
    a, r, c = (arena((1, 8, torch.float32), gpu, poison) for _ in range(3))
    zeros = torch.zeros(9, dtype=torch.int32, device=gpu)
    x = torch.ones(8, device=gpu)
    p = x.data_ptr()
    assert lib.maxk_gat_attention_forward(zeros.data_ptr(), p, p, p, 0.2, a.ptr, 8, 8, 0,
                                          _stream()) == 0
    assert lib.maxk_gat_attention_backward(zeros.data_ptr(), p, p, p, 0.2, p, p, a.ptr, r.ptr, 8,
                                           8, 0, _stream()) == 0
    assert lib.maxk_edge_colsum(zeros.data_ptr(), p, p, c.ptr, 8, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((a.buf == poison).all())
    for x_ in (r, c):
        assert x_.check() is None and bool((x_.payload[0].view(torch.int32) == 0).all())
    r2 = arena((1, 8, torch.float32), gpu, poison)
    assert lib.maxk_gat_attention_backward(zeros.data_ptr(), p, p, p, 0.2, p, p, a.ptr, r2.ptr, 0,
                                           8, 5, _stream()) == 0
    assert lib.maxk_edge_colsum(zeros.data_ptr(), p, p, r2.ptr, 0, 5, _stream()) == 0
    torch.cuda.synchronize()
    assert bool((r2.buf == poison).all()) and bool((a.buf == poison).all())
    e0 = x[:0]
    i0 = zeros[:0]
    assert ops.gat_attention(zeros, i0, x, x, 0.2).shape == (0,)
    ge, ger = ops.gat_attention_backward(zeros, i0, x, x, 0.2, e0, e0)
    assert ge.shape == (0,) and ger.tolist() == [0.0] * 8
    assert ops.edge_colsum(zeros, i0, e0).tolist() == [0.0] * 8


def test_python_checks(gpu):
    ptr, idx, _ = graph_dev(gpu)
    el, er = (dev_of(a, gpu) for a in scores_of(0.5))
    with pytest.raises(RuntimeError, match="er must be \\[num_rows\\]"):
        ops.gat_attention(ptr, idx, el, er[:-1], 0.2)
    with pytest.raises(RuntimeError, match="idx must be int32"):
        ops.gat_attention(ptr, idx.long(), el, er, 0.2)
    with pytest.raises(RuntimeError, match="el must be a CUDA tensor"):
        ops.gat_attention(ptr, idx, el.cpu(), er, 0.2)
    with pytest.raises(RuntimeError, match="grad_alpha must be \\[num_edges\\]"):
        ops.gat_attention_backward(ptr, idx, el, er, 0.2, torch.ones_like(idx, dtype=torch.float32),
                                   er)
    with pytest.raises(RuntimeError, match="values must be \\[num_edges\\]"):
        ops.edge_colsum(ptr, idx, er)
    with pytest.raises(mk.MaxKError, match="negative_slope"):
        ops.gat_attention(ptr, idx, el, er, float("nan"))
    with pytest.raises(mk.MaxKError, match="overlaps"):
        ops.gat_attention_backward(ptr, idx, el, er, 0.2, el[:0].new_ones(idx.numel()),
                                   gvec(gpu, 1), out=(None, er))
    g = mk.CSRGraph(ptr, idx)
    with pytest.raises(RuntimeError, match="el must be a float32"):
        mk.gat_attention(g, el[:-1], er)


# ------------------------------------------------------------------ capture
@pytest.mark.parametrize("poison", POISONS)
def test_capture(gpu, poison):
    """Forward, backward and column sum captured in one graph after an eager call; input contents
    swapped and outputs poisoned between replays; each replay bit-equal to the eager run."""
    ptr, idx, _ = graph_dev(gpu)
    n = ptr.numel() - 1
    pt, order = (dev_of(a, gpu) for a in transposed(graph_arrays()[1], n))
    sets = [scores_of(R) + (np.random.default_rng(s).standard_normal(idx.numel())
                            .astype(np.float32),) for R, s in ((0.5, 20), (60.0, 21), (0.5, 22))]
    eager = []
    for el_np, er_np, g_np in sets:
        el, er = dev_of(el_np, gpu), dev_of(er_np, gpu)
        alpha = ops.gat_attention(ptr, idx, el, er, 0.2)
        ge, ger = ops.gat_attention_backward(ptr, idx, el, er, 0.2, alpha, dev_of(g_np, gpu))
        eager.append([t.cpu().numpy() for t in (alpha, ge, ger, ops.edge_colsum(pt, order, ge))])
    assert (bits(eager[0][0]) != bits(eager[1][0])).mean() > 0.5
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        el, er, g = (dev_of(a, gpu) for a in sets[0])
        outs = [torch.empty_like(g), torch.empty_like(g), torch.empty_like(er),
                torch.empty_like(el)]

        def step():
            ops.gat_attention(ptr, idx, el, er, 0.2, out=outs[0])
            ops.gat_attention_backward(ptr, idx, el, er, 0.2, outs[0], g, out=(outs[1], outs[2]))
            ops.edge_colsum(pt, order, outs[1], out=outs[3])

        step()
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            step()
        for i in (1, 2, 1):
            for t, a in zip((el, er, g), sets[i]):
                t.copy_(dev_of(a, gpu))
            for o in outs:
                o.view(torch.uint8).fill_(poison)
            graph.replay()
            s.synchronize()
            for o, want, what in zip(outs, eager[i], ("alpha", "grad_edge", "grad_er", "grad_el")):
                assert_same_bits(o.cpu().numpy(), want, f"replay of set {i}: {what}")
    del graph
    torch.cuda.synchronize()


# ------------------------------------------------------------------ autograd, operators
def _graph(dev):
    ptr, idx = graph_arrays()
    return mk.CSRGraph(dev_of(ptr, dev), dev_of(idx, dev))


def _fn_surface(graph, el, er, slope=0.2):
    return mk.gat_attention(graph, el, er, slope)


def _op_surface(graph, el, er, slope=0.2):
    return torch.ops.maxk.gat_attention(graph.ptr, graph.idx, graph.transposed_structure()[0],
                                        graph.transposed_order(), el, er, slope)


SURFACES = [pytest.param(_fn_surface, id="function"), pytest.param(_op_surface, id="operator")]


def _leaves(dev, R=0.5):
    return [dev_of(a, dev).requires_grad_(True) for a in scores_of(R)]


def _check_grads(graph, el, er, alpha, g, grad_el, grad_er, what, slope=0.2):
    """alpha bit for bit with the composition; grad_edge is defined bit for bit from (alpha, g),
    and the two gradients are its row and column sums within the derived bounds."""
    ptr_np, idx_np = graph_arrays()
    rows = graph.edge_rows()
    with torch.no_grad():
        want = composition(graph.ptr, graph.idx, rows, el, er, slope)
        assert_same_bits(alpha.detach().cpu().numpy(), want.cpu().numpy(), what + ": alpha")
        ge = grad_edge_composition(graph.ptr, graph.idx, rows, el, er, slope, want,
                                   g.contiguous()).cpu().numpy()
    n = ptr_np.size - 1
    if grad_er is not None:
        worst_by_length(np.abs(grad_er.cpu().numpy().astype(np.float64) - row_sums64(ptr_np, ge)),
                        row_sum_bound(ptr_np, ge), np.diff(ptr_np), what + ": grad_er")
    if grad_el is not None:
        worst_by_length(np.abs(grad_el.cpu().numpy().astype(np.float64) -
                               col_sums64(idx_np, ge, n)),
                        col_sum_bound(idx_np, ge, n), np.bincount(idx_np, minlength=n),
                        what + ": grad_el")


@pytest.mark.parametrize("surface", SURFACES)
def test_autograd_gradients_repeated_and_accumulated(gpu, surface):
    graph = _graph(gpu)
    el, er = _leaves(gpu)
    g1, g2 = gvec(gpu, 31), gvec(gpu, 32)
    alpha = surface(graph, el, er)
    if surface is _fn_surface:
        assert sorted(t.numel() for t in alpha.grad_fn.saved_tensors) == sorted(
            [alpha.numel(), el.numel(), er.numel()])
    alpha.backward(g1, retain_graph=True)
    once = (el.grad.clone(), er.grad.clone())
    _check_grads(graph, el, er, alpha, g1, *once, "one backward")
    alpha.backward(g1)                                   # again through the retained graph
    for got, one in zip((el.grad, er.grad), once):
        assert_same_bits(got.cpu().numpy(), (one + one).cpu().numpy(), "two backwards")
    # a second step with another gradient accumulates onto the first
    el2, er2 = _leaves(gpu)
    surface(graph, el2, er2).backward(g1)
    surface(graph, el2, er2).backward(g2)
    el3, er3 = _leaves(gpu)
    surface(graph, el3, er3).backward(g2)
    for got, one, two in zip((el2.grad, er2.grad), once, (el3.grad, er3.grad)):
        assert_same_bits(got.cpu().numpy(), (one + two).cpu().numpy(), "accumulated over two steps")


@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("need", ["el", "er", "neither"])
def test_only_the_needed_kernels_run(gpu, monkeypatch, surface, need):
    graph = _graph(gpu)
    graph.transposed_order()
    calls = []
    for name in ("gat_attention_backward", "edge_colsum"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _r=real, _n=name, **k: calls.append(_n) or
                            _r(*a, **k))
    real_order = mk.CSRGraph.transposed_order
    monkeypatch.setattr(mk.CSRGraph, "transposed_order",
                        lambda self: calls.append("order") or real_order(self))
    el, er = _leaves(gpu)
    el.requires_grad_(need == "el")
    er.requires_grad_(need == "er")
    if surface is _op_surface:
        pt, order = graph.transposed_structure()[0], real_order(graph)
        alpha = torch.ops.maxk.gat_attention(graph.ptr, graph.idx, pt, order, el, er, 0.2)
    else:
        alpha = surface(graph, el, er)
    g = gvec(gpu, 33)
    if need == "neither":
        assert not alpha.requires_grad and alpha.grad_fn is None
        w = torch.ones_like(alpha, requires_grad=True)
        (alpha * w).sum().backward()
        assert calls == [] and w.grad is not None
        return
    alpha.backward(g)
    if need == "er":
        assert calls == ["gat_attention_backward"] and el.grad is None
        _check_grads(graph, el, er, alpha, g, None, er.grad, "only er")
    else:
        want = ["gat_attention_backward"] + (["order"] if surface is _fn_surface else []) + \
            ["edge_colsum"]
        assert calls == want and er.grad is None
        _check_grads(graph, el, er, alpha, g, el.grad, None, "only el")


@pytest.mark.parametrize("surface", SURFACES)
def test_create_graph_raises_on_the_second_differentiation(gpu, surface):
    graph = _graph(gpu)
    el, er = _leaves(gpu)
    g = gvec(gpu, 34)
    alpha = surface(graph, el, er)
    got = torch.autograd.grad(alpha, [el, er], g, create_graph=True)
    _check_grads(graph, el, er, alpha, g, got[0].detach(), got[1].detach(), "create_graph")
    for t in got:
        assert t.requires_grad
        with pytest.raises(RuntimeError, match=r"differentiate twice|once_differentiable"):
            t.sum().backward()


@pytest.mark.parametrize("surface", SURFACES)
@pytest.mark.parametrize("reentrant", [False, True])
def test_checkpoint(gpu, surface, reentrant):
    graph = _graph(gpu)
    g = gvec(gpu, 35)
    el, er = _leaves(gpu)
    plain = surface(graph, el, er)
    plain.backward(g)
    el2, er2 = _leaves(gpu)
    out = checkpoint(lambda a, b: surface(graph, a, b), el2, er2, use_reentrant=reentrant)
    assert torch.equal(out.detach(), plain.detach())
    out.backward(g)
    assert torch.equal(el2.grad, el.grad) and torch.equal(er2.grad, er.grad)
    _check_grads(graph, el2, er2, out, g, el2.grad, er2.grad, f"checkpoint({reentrant})")


@pytest.mark.parametrize("surface", SURFACES)
def test_no_grad_strided_gradient_views_and_inplace_edit(gpu, surface):
    graph = _graph(gpu)
    n, e = graph.num_nodes, graph.num_edges
    el, er = _leaves(gpu)
    with torch.no_grad():
        alpha = surface(graph, el, er)
    assert not alpha.requires_grad and alpha.grad_fn is None
    # a strided incoming gradient: every second element of a longer tensor
    wide = gvec(gpu, 36, 2 * e)
    alpha = surface(graph, el, er)
    alpha.backward(wide[::2])
    _check_grads(graph, el, er, alpha, wide[::2], el.grad, er.grad, "strided gradient")
    # el and er as views of one leaf
    leaf = torch.cat([t.detach() for t in (el, er)]).requires_grad_(True)
    g = gvec(gpu, 37)
    alpha = surface(graph, leaf[:n], leaf[n:])
    alpha.backward(g)
    _check_grads(graph, leaf.detach()[:n], leaf.detach()[n:], alpha, g, leaf.grad[:n],
                 leaf.grad[n:], "views of one leaf")
    # an in-place edit of el between forward and backward
    el2 = el.detach().clone().requires_grad_(True)
    work = el2 * 1.0
    alpha = surface(graph, work, er)
    work.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        alpha.backward(g)


def test_operator_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        ptr = torch.empty(51, dtype=torch.int32, device="cuda")
        pt = torch.empty(41, dtype=torch.int32, device="cuda")
        idx = torch.empty(300, dtype=torch.int32, device="cuda")
        el, er, x = (torch.empty(k, device="cuda") for k in (40, 50, 300))
        out = torch.ops.maxk.gat_attention(ptr, idx, pt, idx, el, er, 0.2)
        assert out.shape == (300,) and out.dtype == torch.float32 and out.device.type == "cuda"
        ge, ger = torch.ops.maxk.gat_attention_backward(ptr, idx, el, er, 0.2, x, x)
        assert ge.shape == (300,) and ger.shape == (50,) and ger.dtype == torch.float32
        assert torch.ops.maxk.edge_colsum(pt, idx, x).shape == (40,)


def test_operator_opcheck_and_compile(gpu):
    """torch.compile(fullgraph=True) keeps the operator as one node; compiled and eager steps
    agree bit for bit, gradients included."""
    graph = _graph(gpu)
    pt, order = graph.transposed_structure()[0], graph.transposed_order()
    el, er = _leaves(gpu)
    w = gvec(gpu, 40)
    torch.library.opcheck(torch.ops.maxk.gat_attention.default,
                          (graph.ptr, graph.idx, pt, order, el, er, 0.2))
    seen = []

    def backend(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == "call_function")
        return gm.forward

    def step(ptr, idx, pt, order, el, er, w):
        return (torch.ops.maxk.gat_attention(ptr, idx, pt, order, el, er, 0.2) * w).sum()

    le = step(graph.ptr, graph.idx, pt, order, el, er, w)
    le.backward()
    el2, er2 = _leaves(gpu)
    lc = torch.compile(step, backend=backend, fullgraph=True)(graph.ptr, graph.idx, pt, order, el2,
                                                              er2, w)
    lc.backward()
    assert any("gat_attention" in t for t in seen) and not any("leaky" in t for t in seen), seen
    assert torch.equal(le.detach(), lc.detach())
    assert_same_bits(el2.grad.cpu().numpy(), el.grad.cpu().numpy(), "compiled step: grad_el")
    assert_same_bits(er2.grad.cpu().numpy(), er.grad.cpu().numpy(), "compiled step: grad_er")
    assert attention.GATAttentionFunction.__module__ == "maxk_kernels.attention"


# ------------------------------------------------------------------ MaxKGATConv
def _layer(dev, nonlinear, train, fused):
    torch.manual_seed(3)
    layer = mk.MaxKGATConv(tges.D_L, tges.D_L, maxk=tges.K_L, nonlinear=nonlinear,
                           fused_dropout=True, feat_drop=0.5 if train else 0.0,
                           fused_attention=fused).to(dev)
    with torch.no_grad():
        layer.bias.copy_(tges._randn(dev, (tges.D_L,), 50))
    return layer.train(train)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("nonlinear", ["maxk", "relu"])
def test_gat_layer_output_is_bit_identical_with_and_without_fusion(gpu, nonlinear, train):
    g = tges._gat_graph(gpu)
    feat = tges._randn(gpu, (tges.N_L, tges.D_L), 51)
    outs = []
    for fused in (False, True):
        layer = _layer(gpu, nonlinear, train, fused)
        assert layer.fused_attention is fused
        torch.manual_seed(77)
        outs.append(layer(g, feat).detach().cpu().numpy())
    assert float(np.abs(outs[0]).sum()) > 0
    assert_same_bits(outs[1], outs[0], f"{nonlinear} train={train}")


@pytest.mark.parametrize("nonlinear", ["maxk", "relu"])
def test_fused_gat_layer_against_the_dense_float64_restatement(gpu, monkeypatch, nonlinear):
    """The restatement and the bounds test_gpu_edge_softmax.py holds the unfused layer to, run on
    the fused one: its bounds on the score gradients hold for a sum in any order."""
    calls = []
    for name in ("gat_attention", "gat_attention_backward", "edge_colsum"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _r=real, _n=name, **k: calls.append(_n) or
                            _r(*a, **k))
    monkeypatch.setattr(tges, "_gat_layer", lambda dev, nl, train: _layer(dev, nl, train, True))
    tges.test_gat_layer_against_a_dense_float64_restatement(gpu, nonlinear)
    assert calls == ["gat_attention", "gat_attention_backward", "edge_colsum"]


def test_unfused_gat_layer_calls_none_of_the_new_functions(gpu, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a fused-attention function ran with fused_attention=False")

    for name in ("gat_attention", "gat_attention_backward", "edge_colsum"):
        monkeypatch.setattr(ops, name, refuse)
    monkeypatch.setattr(mk.CSRGraph, "transposed_order", refuse)
    g = tges._gat_graph(gpu)
    layer = mk.MaxKGATConv(tges.D_L, tges.D_L, maxk=tges.K_L).to(gpu)
    assert layer.fused_attention is False
    feat = tges._randn(gpu, (tges.N_L, tges.D_L), 51).requires_grad_(True)
    layer(g, feat).sum().backward()
    assert feat.grad is not None and layer.attn_l.grad is not None
