"""GPU: maxk_edge_softmax_forward / _backward against the float64 restatement and the error
bounds of test_edge_softmax_capi.py (include/maxk_hip.h, "Edge softmax"), their output
contract, graph capture, the autograd Function, the registered operators, CSRGraph.edge_rows and
the MaxKGATConv layer built on them.

Row lengths straddle every regime limit the library reports (ops.edge_softmax_row_limits), so
nothing here hard-codes them. One graph (LAYOUT) serves most tests: every length of LENGTHS four
times, behind a filler row of 0 .. 3 edges chosen so that the row's segment starts at every
residue mod 4; the fillers are the empty (and 1 .. 3 edge) rows in between."""
import functools

import numpy as np
import pytest
import torch

import maxk_kernels as mk
from arena import POISONS, arena
from maxk_kernels import _lib, ops
from test_edge_softmax_capi import (backward_bound, forward_bound, softmax_backward_rows64,
                                    softmax_rows64)

pytestmark = pytest.mark.gpu

LIMITS = ops.edge_softmax_row_limits()
HUB = max(2 * max(LIMITS) + 1, 5000)
LENGTHS = sorted({0, 1, 2, 3, 63, 64, 65, 127, 128, 129, HUB} |
                 {L + d for L in LIMITS for d in (-1, 0, 1)})
REGIMES = len(LIMITS) + 1


def regime(n):
    """Which regime serves a row of n edges: a row of exactly a limit's length the lower one."""
    return sum(n > L for L in LIMITS)


@functools.lru_cache(maxsize=None)
def layout():
    """(deg int64 [rows], [(row, n, start % 4)] of the rows placed on purpose)."""
    deg, placed, cur = [], [], 0
    for n in LENGTHS:
        for q in range(4):
            f = (q - cur) % 4
            deg.append(f)
            cur += f
            placed.append((len(deg), n, cur % 4))
            deg.append(n)
            cur += n
    assert {(n, q) for _, n, q in placed} == {(n, q) for n in LENGTHS for q in range(4)}
    assert 0 in deg and all(regime(n) < REGIMES for n in LENGTHS)
    assert {regime(n) for n in LENGTHS if n} == set(range(REGIMES))
    return np.asarray(deg, dtype=np.int64), placed


def ptr_of(deg):
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def logits_of(R, seed=5):
    """Random logits in [0, R) for LAYOUT, with their float64 softmax and bound (shared)."""
    deg, _ = layout()
    x = (np.random.default_rng(seed).random(int(deg.sum())) * R).astype(np.float32)
    ptr = ptr_of(deg)
    y64, bound = softmax_rows64(ptr, x), forward_bound(ptr, x)
    for a in (x, y64, bound):
        a.setflags(write=False)
    return ptr, x, y64, bound


def dev_of(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def fwd(dev, ptr, x):
    out = ops.edge_softmax(dev_of(ptr, dev), dev_of(x, dev))
    return out.cpu().numpy()


def bwd(dev, ptr, y, g):
    out = ops.edge_softmax_backward(dev_of(ptr, dev), dev_of(y, dev), dev_of(g, dev))
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    diff = np.flatnonzero(bits(got) != bits(want))
    assert diff.size == 0, (f"{what}: {diff.size} of {got.size} differ, first at {diff[0]}: "
                            f"got {got[diff[0]]!r}, want {want[diff[0]]!r}")


def edge_regime(ptr):
    return np.repeat([regime(n) for n in np.diff(ptr)], np.diff(ptr))


def worst_ratio(err, bound, ptr, what):
    """Prints the worst error / bound per regime (pytest -s) and asserts it is <= 1."""
    ratio = err / bound
    reg = edge_regime(ptr)
    worst = [float(ratio[reg == r].max()) for r in range(REGIMES)]
    print(f"\n{what}: worst error / bound per regime {['%.3f' % w for w in worst]}")
    assert np.isfinite(ratio).all() and max(worst) <= 1.0, (what, worst)


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("R", [0.5, 16.0, 60.0])
def test_forward_and_backward_within_their_bounds(gpu, R):
    """|out - y64| <= (2 R + ceil(n / 64) + 20) u y64 + 2^-126 with R the row's own range; at
    R <= 0.5 that is about 100 u at the hub row, so one edge dropped or doubled out of its 5,000
    (2e-4 relative) fails. The backward runs on the kernel's own f32 output and is held to
    (ceil(n / 64) + 10) u y (|g| + sum |y g|) + 2^-126 against float64 on those f32 inputs."""
    ptr, x, y64, bound = logits_of(R)
    got = fwd(gpu, ptr, x)
    assert got.dtype == np.float32 and got.shape == x.shape
    worst_ratio(np.abs(got.astype(np.float64) - y64), bound, ptr, f"forward R={R}")
    g = np.random.default_rng(6).standard_normal(x.size).astype(np.float32)
    grad = bwd(gpu, ptr, got, g)
    worst_ratio(np.abs(grad.astype(np.float64) - softmax_backward_rows64(ptr, got, g)),
                backward_bound(ptr, got, g), ptr, f"backward R={R}")


def test_exact_rows(gpu):
    """All-equal logits give fl32(1 / n) bit for bit (p = 1 exactly, the sum n exactly, one
    correctly rounded reciprocal); logits in {0, -Inf} give fl32(1 / count) and +0.0f, and the
    -Inf edges a zero gradient."""
    deg, _ = layout()
    ptr = ptr_of(deg)
    rows = np.repeat(np.arange(deg.size), deg)
    n_of = deg[rows]
    x = (rows % 7 * 0.375 - 1.0).astype(np.float32)              # one constant per row
    assert_same_bits(fwd(gpu, ptr, x), np.float32(1) / n_of.astype(np.float32), "all equal")
    rng = np.random.default_rng(8)
    keep = rng.random(rows.size) < 0.5
    keep[ptr[:-1][deg > 0] + rng.integers(0, 1 << 30, int((deg > 0).sum())) % deg[deg > 0]] = True
    count = np.zeros(deg.size)
    np.add.at(count, rows, keep)
    x = np.where(keep, np.float32(0), np.float32(-np.inf)).astype(np.float32)
    want = np.where(keep, np.float32(1) / count[rows].astype(np.float32), np.float32(0))
    got = fwd(gpu, ptr, x)
    assert_same_bits(got, want.astype(np.float32), "{0, -Inf}")
    g = rng.standard_normal(rows.size).astype(np.float32)
    grad = bwd(gpu, ptr, got, g)
    assert np.all(grad[~keep] == 0)
    worst_ratio(np.abs(grad.astype(np.float64) - softmax_backward_rows64(ptr, got, g)),
                backward_bound(ptr, got, g), ptr, "backward {0, -Inf}")


def test_non_finite_rows(gpu):
    """One row each with a NaN, a +Inf and only -Inf, in every regime: those rows are NaN
    throughout, forward and backward, and every other row keeps the bits of the clean run."""
    ptr, x, _, _ = logits_of(0.5)
    deg, placed = layout()
    x2 = x.copy()
    hit = np.zeros(deg.size, dtype=bool)
    for r in range(REGIMES):
        rows = [row for row, n, _ in placed if n > 1 and regime(n) == r]
        assert len(rows) >= 3
        for kind, row in zip(("nan", "inf", "ninf"), (rows[0], rows[len(rows) // 2], rows[-1])):
            b, e = int(ptr[row]), int(ptr[row + 1])
            if kind == "nan":
                x2[b + (e - b) // 2] = np.nan
            elif kind == "inf":
                x2[e - 1] = np.inf
            else:
                x2[b:e] = -np.inf
            hit[row] = True
    bad = np.repeat(hit, deg)
    g = np.random.default_rng(9).standard_normal(x.size).astype(np.float32)
    clean, dirty = fwd(gpu, ptr, x), fwd(gpu, ptr, x2)
    assert np.isnan(dirty[bad]).all() and np.isnan(softmax_rows64(ptr, x2)[bad]).all()
    assert_same_bits(dirty[~bad], clean[~bad], "forward, rows beside non-finite ones")
    gc, gd = bwd(gpu, ptr, clean, g), bwd(gpu, ptr, dirty, g)
    assert np.isnan(gd[bad]).all()
    assert_same_bits(gd[~bad], gc[~bad], "backward, rows beside non-finite ones")


def _per_row(ptr, a):
    return [a[ptr[r]:ptr[r + 1]] for r in range(ptr.size - 1)]


def test_position_independence(gpu):
    """The same rows in reversed order, and behind one more 1-edge row (every segment start
    moves by one), give the same bits per row, forward and backward."""
    ptr, x, _, _ = logits_of(16.0)
    deg, _ = layout()
    g = np.random.default_rng(10).standard_normal(x.size).astype(np.float32)
    y = fwd(gpu, ptr, x)
    gr = bwd(gpu, ptr, y, g)
    xs, gs, ys, grs = (_per_row(ptr, a) for a in (x, g, y, gr))
    for what, order, lead in [("reversed", list(range(deg.size - 1, -1, -1)), 0),
                              ("shifted", list(range(deg.size)), 1)]:
        def cat(parts, first):
            return np.concatenate([np.float32([first])] * lead + [parts[r] for r in order])

        p2 = ptr_of([1] * lead + [int(deg[r]) for r in order])
        y2 = fwd(gpu, p2, cat(xs, 0.25))
        assert_same_bits(y2, cat(ys, 1.0), what)             # a 1-edge row is exactly 1
        g2 = bwd(gpu, p2, y2, cat(gs, 3.0))
        assert_same_bits(g2, cat(grs, 0.0), what + " backward")   # and its gradient 1 * (3 - 3)


# ------------------------------------------------------------------ output contract
def _raw_fwd(ptr, x, out_ptr, n=None, e=None):
    return _lib.lib.maxk_edge_softmax_forward(
        ptr.data_ptr(), x.data_ptr(), out_ptr, ptr.numel() - 1 if n is None else n,
        x.numel() if e is None else e, torch.cuda.current_stream().cuda_stream)


def _raw_bwd(ptr, y, g, out_ptr, n=None, e=None):
    return _lib.lib.maxk_edge_softmax_backward(
        ptr.data_ptr(), y.data_ptr(), g.data_ptr(), out_ptr, ptr.numel() - 1 if n is None else n,
        y.numel() if e is None else e, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("poison", POISONS)
def test_outputs_are_fully_overwritten_and_nothing_else(gpu, poison):
    ptr_np, x_np, _, _ = logits_of(16.0)
    ptr, x = dev_of(ptr_np, gpu), dev_of(x_np, gpu)
    g = dev_of(np.random.default_rng(11).standard_normal(x_np.size).astype(np.float32), gpu)
    keep = [t.clone() for t in (ptr, x, g)]
    a = arena((1, x.numel(), torch.float32), gpu, poison)
    assert _raw_fwd(ptr, x, a.ptr) == 0
    torch.cuda.synchronize()
    assert a.check() is None and a.first_poisoned() is None
    y = a.payload[0].clone()
    assert_same_bits(y.cpu().numpy(), fwd(gpu, ptr_np, x_np), "arena forward")
    b = arena((1, x.numel(), torch.float32), gpu, poison)
    assert _raw_bwd(ptr, y, g, b.ptr) == 0
    torch.cuda.synchronize()
    assert b.check() is None and b.first_poisoned() is None
    assert_same_bits(b.payload[0].cpu().numpy(), bwd(gpu, ptr_np, y.cpu().numpy(), g.cpu().numpy()),
                     "arena backward")
    assert a.check() is None and torch.equal(a.payload[0], y)     # the backward's input
    for t, k in zip((ptr, x, g), keep):
        assert torch.equal(t, k)


@pytest.mark.parametrize("poison", POISONS)
def test_empty_calls_write_nothing(gpu, poison):
    a = arena((1, 64, torch.float32), gpu, poison)
    zeros = torch.zeros(9, dtype=torch.int32, device=gpu)
    x = torch.ones(64, device=gpu)
    for n, e in [(8, 0), (0, 0), (0, 64)]:
        assert _raw_fwd(zeros, x, a.ptr, n=n, e=e) == 0
        assert _raw_bwd(zeros, x, x, a.ptr, n=n, e=e) == 0
    # rows, edges, and every row empty but the last (ptr[num_rows] == num_edges holds)
    ptr = torch.tensor([0] * 8 + [3], dtype=torch.int32, device=gpu)
    b = arena((1, 3, torch.float32), gpu, poison)
    assert _raw_fwd(ptr, x[:3], b.ptr) == 0
    torch.cuda.synchronize()
    assert bool((a.buf == poison).all())
    assert b.check() is None and b.payload[0].tolist() == [float(np.float32(1) / np.float32(3))] * 3
    assert ops.edge_softmax(zeros, x[:0]).shape == (0,)
    assert ops.edge_softmax_backward(zeros[:1], x[:0], x[:0]).shape == (0,)


def _shift(t):
    """The same values as a contiguous view one element into a larger buffer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t)
    return buf[1:]


def test_views_one_element_into_a_buffer(gpu):
    """Arrays need only element alignment: every pointer in turn 4 B off its allocation."""
    ptr_np, x_np, _, _ = logits_of(16.0)
    ptr, x = dev_of(ptr_np, gpu), dev_of(x_np, gpu)
    g = dev_of(np.random.default_rng(12).standard_normal(x_np.size).astype(np.float32), gpu)
    y = ops.edge_softmax(ptr, x)
    gr = ops.edge_softmax_backward(ptr, y, g)
    for which in ("ptr", "logits", "out"):
        out = _shift(torch.empty_like(x)) if which == "out" else None
        got = ops.edge_softmax(_shift(ptr) if which == "ptr" else ptr,
                               _shift(x) if which == "logits" else x, out=out)
        assert got.data_ptr() % 16 == (4 if which == "out" else 0)
        assert_same_bits(got.cpu().numpy(), y.cpu().numpy(), f"forward, {which} shifted")
    for which in ("ptr", "y", "grad_y", "out"):
        out = _shift(torch.empty_like(x)) if which == "out" else None
        got = ops.edge_softmax_backward(_shift(ptr) if which == "ptr" else ptr,
                                        _shift(y) if which == "y" else y,
                                        _shift(g) if which == "grad_y" else g, out=out)
        assert_same_bits(got.cpu().numpy(), gr.cpu().numpy(), f"backward, {which} shifted")


def test_adjacent_ranges_are_accepted(gpu):
    """The overlap check refuses shared bytes only: output directly behind, and directly in
    front of, its input in one allocation."""
    ptr_np, x_np, _, _ = logits_of(0.5)
    ptr, e = dev_of(ptr_np, gpu), x_np.size
    want = fwd(gpu, ptr_np, x_np)
    for first in (True, False):
        buf = torch.empty(2 * e, device=gpu)
        x, out = (buf[:e], buf[e:]) if first else (buf[e:], buf[:e])
        x.copy_(dev_of(x_np, gpu))
        assert_same_bits(ops.edge_softmax(ptr, x, out=out).cpu().numpy(), want, "adjacent")
        with pytest.raises(mk.MaxKError, match="overlaps"):
            ops.edge_softmax(ptr, x, out=buf[1:e + 1] if first else buf[e - 1:2 * e - 1])


def test_repeated_calls_are_bitwise_equal(gpu):
    ptr_np, x_np, _, _ = logits_of(60.0)
    ptr, x = dev_of(ptr_np, gpu), dev_of(x_np, gpu)
    g = dev_of(np.random.default_rng(13).standard_normal(x_np.size).astype(np.float32), gpu)
    y1, y2 = ops.edge_softmax(ptr, x), ops.edge_softmax(ptr, x)
    g1, g2 = ops.edge_softmax_backward(ptr, y1, g), ops.edge_softmax_backward(ptr, y1, g)
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))


@pytest.mark.parametrize("poison", POISONS)
def test_capture(gpu, poison):
    """Forward and backward captured after one eager call; inputs swapped and outputs poisoned
    between two replays; each replay bit-equal to the eager run of the same inputs."""
    ptr_np = logits_of(0.5)[0]
    sets = [(logits_of(R)[1], np.random.default_rng(s).standard_normal(ptr_np[-1])
             .astype(np.float32)) for R, s in ((0.5, 20), (16.0, 21), (60.0, 22))]
    ptr = dev_of(ptr_np, gpu)
    eager = []
    for x_np, g_np in sets:
        y = ops.edge_softmax(ptr, dev_of(x_np, gpu))
        eager.append((y.cpu().numpy(),
                      ops.edge_softmax_backward(ptr, y, dev_of(g_np, gpu)).cpu().numpy()))
    assert (bits(eager[0][0]) != bits(eager[1][0])).mean() > 0.5
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x, g = dev_of(sets[0][0], gpu), dev_of(sets[0][1], gpu)
        y, gr = torch.empty_like(x), torch.empty_like(x)

        def step():
            ops.edge_softmax(ptr, x, out=y)
            ops.edge_softmax_backward(ptr, y, g, out=gr)

        step()
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            step()
        for i in (1, 2, 1):
            x.copy_(dev_of(sets[i][0], gpu))
            g.copy_(dev_of(sets[i][1], gpu))
            y.view(torch.uint8).fill_(poison)
            gr.view(torch.uint8).fill_(poison)
            graph.replay()
            s.synchronize()
            assert_same_bits(y.cpu().numpy(), eager[i][0], f"replay of set {i}, forward")
            assert_same_bits(gr.cpu().numpy(), eager[i][1], f"replay of set {i}, backward")
    del graph
    torch.cuda.synchronize()


# ------------------------------------------------------------------ autograd, operators
def _layout_graph(dev):
    deg, _ = layout()
    ptr = ptr_of(deg)
    idx = np.random.default_rng(30).integers(0, deg.size, int(ptr[-1])).astype(np.int32)
    return mk.CSRGraph(dev_of(ptr, dev), dev_of(idx, dev))


def test_autograd_gradient_within_bound(gpu):
    """loss = sum w_e alpha_e, so grad_y = w. The kernel's gradient is its backward on its own
    f32 output yh: within backward_bound(yh, w) of the exact gradient of yh. The exact gradient
    moves with the forward's error: yh_e = y_e (1 + d_e), |d_e| <= eps = forward_bound / y (the
    2^-126 term included), so with t = sum y w, S = sum |y w| and
    tau = sum d y w (|tau| <= eps S, |t| <= S):
        yh_e (w_e - t - tau) - y_e (w_e - t) = y_e d_e (w_e - t) - y_e (1 + d_e) tau
        |...| <= y_e eps (|w_e| + S) + y_e (1 + eps) eps S <= eps (1 + eps) y_e (|w_e| + 2 S),
    eps taken as the row's largest. The two add up."""
    ptr, x, y64, _ = logits_of(16.0)
    graph = _layout_graph(gpu)
    w = np.random.default_rng(31).standard_normal(x.size).astype(np.float32)
    logits = dev_of(x, gpu).requires_grad_(True)
    alpha = mk.edge_softmax(graph, logits)
    assert alpha.grad_fn is not None and [t.shape for t in alpha.grad_fn.saved_tensors] == [x.shape]
    (alpha * dev_of(w, gpu)).sum().backward()
    yh = alpha.detach().cpu().numpy()
    assert_same_bits(yh, fwd(gpu, ptr, x), "autograd forward")
    w64 = w.astype(np.float64)
    rows = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    S = np.zeros(ptr.size - 1)
    np.add.at(S, rows, np.abs(y64 * w64))
    eps = np.zeros(ptr.size - 1)
    np.maximum.at(eps, rows, forward_bound(ptr, x) / y64)     # relative, 2^-126 included
    eps = eps[rows]
    carried = eps * (1 + eps) * y64 * (np.abs(w64) + 2 * S[rows])
    t = np.zeros(ptr.size - 1)
    np.add.at(t, rows, y64 * w64)
    ref = y64 * (w64 - t[rows])
    worst_ratio(np.abs(logits.grad.cpu().numpy().astype(np.float64) - ref),
                backward_bound(ptr, yh, w) + carried, ptr, "autograd gradient")


def test_no_gradient_kernel_without_a_gradient_to_compute(gpu, monkeypatch):
    graph = _layout_graph(gpu)
    calls = []
    real = ops.edge_softmax_backward
    monkeypatch.setattr(ops, "edge_softmax_backward",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    x = dev_of(logits_of(0.5)[1], gpu)
    alpha = mk.edge_softmax(graph, x)
    assert not alpha.requires_grad and alpha.grad_fn is None
    w = torch.ones_like(x, requires_grad=True)
    (alpha * w).sum().backward()
    assert calls == [] and w.grad is not None
    xg = x.clone().requires_grad_(True)
    mk.edge_softmax(graph, xg).sum().backward()
    assert calls == [1]
    with pytest.raises(RuntimeError, match="logits"):
        mk.edge_softmax(graph, x[:-1])


def test_operator_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        ptr = torch.empty(51, dtype=torch.int32, device="cuda")
        x = torch.empty(300, device="cuda")
        for out in (torch.ops.maxk.edge_softmax(ptr, x),
                    torch.ops.maxk.edge_softmax_backward(ptr, x, x)):
            assert out.shape == (300,) and out.dtype == torch.float32 and out.device.type == "cuda"


def test_operators_opcheck_compile_and_differentiate(gpu):
    ptr_np, x_np, _, _ = logits_of(16.0)
    ptr, x = dev_of(ptr_np, gpu), dev_of(x_np, gpu)
    w = dev_of(np.random.default_rng(40).standard_normal(x_np.size).astype(np.float32), gpu)
    y = ops.edge_softmax(ptr, x)
    torch.library.opcheck(torch.ops.maxk.edge_softmax.default, (ptr, x.clone().requires_grad_(True)))
    torch.library.opcheck(torch.ops.maxk.edge_softmax_backward.default, (ptr, y, w))
    seen = []

    def backend(gm, example_inputs):
        seen.extend(str(n.target) for n in gm.graph.nodes if n.op == "call_function")
        return gm.forward

    def step(ptr, x, w):
        return (torch.ops.maxk.edge_softmax(ptr, x) * w).sum()

    xe, xc = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    le = step(ptr, xe, w)
    le.backward()
    lc = torch.compile(step, backend=backend, fullgraph=True)(ptr, xc, w)
    lc.backward()
    assert any("edge_softmax" in t for t in seen), seen
    assert torch.equal(le.detach(), lc.detach())
    assert_same_bits(xc.grad.cpu().numpy(), xe.grad.cpu().numpy(), "compiled step gradient")
    assert_same_bits(xe.grad.cpu().numpy(), ops.edge_softmax_backward(ptr, y, w).cpu().numpy(),
                     "registered derivative")
    fn = torch.compile(lambda *a: torch.ops.maxk.edge_softmax_backward(*a) * 1.0, backend=backend,
                       fullgraph=True)
    assert_same_bits(fn(ptr, y, w).cpu().numpy(), xe.grad.cpu().numpy(), "compiled backward op")
    assert any("edge_softmax_backward" in t for t in seen), seen


def test_edge_rows_is_the_repeat_interleave_and_is_computed_once(gpu, monkeypatch):
    graph = _layout_graph(gpu)
    want = torch.repeat_interleave(torch.arange(graph.num_nodes, device=gpu), graph.in_degrees())
    calls = []
    real = torch.repeat_interleave
    monkeypatch.setattr(torch, "repeat_interleave",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    rows = graph.edge_rows()
    assert rows.dtype == torch.int64 and torch.equal(rows, want)
    assert graph.edge_rows() is rows and calls == [1]


# ------------------------------------------------------------------ MaxKGATConv
N_L, E_L, D_L, K_L = 300, 3000, 64, 16     # the sizes of test_gpu_edge_grad.py's layer tests


def _gat_graph(dev):
    from maxk_kernels import graphs
    ptr, idx = graphs.synthetic_csr(N_L, E_L, seed=21)
    return mk.CSRGraph(ptr.to(dev), idx.to(dev))


def _randn(dev, shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _gat_layer(dev, nonlinear, train):
    torch.manual_seed(3)
    layer = mk.MaxKGATConv(D_L, D_L, maxk=K_L, nonlinear=nonlinear, fused_dropout=True,
                           feat_drop=0.5 if train else 0.0).to(dev)
    with torch.no_grad():
        layer.bias.copy_(_randn(dev, (D_L,), 50))
    return layer.train(train)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("nonlinear", ["maxk", "relu"])
def test_gat_layer_is_the_composition_of_the_public_functions(gpu, nonlinear, train):
    """Output and every parameter and input gradient bit-equal to the layer's forward written out
    by hand with the public functions, in eval mode and in training with fused feature dropout
    under a fixed seed (the drawn seed and F.dropout's mask repeat under torch.manual_seed).

    The SSpMM backward adds a column's terms alpha_e * gout[r, f] with f32 LDS atomics in no
    fixed order (tests/test_gpu_edge_grad.py, "exactly summable"), and attention weights lie on
    no grid that would make such a sum exact. So the upstream gradient is random normal on rows
    whose in-neighbourhoods are pairwise disjoint and zero elsewhere: every column's sum then has
    at most one nonzero term, which is exact in any order, while every operation of the layer
    and every parameter still gets a gradient. Two runs differ by nothing but what the layer
    does."""
    g = _gat_graph(gpu)
    ptr_h, idx_h = g.ptr.cpu().numpy(), g.idx.cpu().numpy()
    used, live = set(), []
    for row in range(N_L):
        cols = set(idx_h[ptr_h[row]:ptr_h[row + 1]].tolist())
        if not cols & used:
            used |= cols
            live.append(row)
    assert len(live) >= 8
    keep = torch.zeros(N_L, 1)
    keep[live] = 1.0
    layer = _gat_layer(gpu, nonlinear, train)
    feat = _randn(gpu, (N_L, D_L), 51).requires_grad_(True)
    gout = (torch.randn((N_L, D_L), generator=torch.Generator().manual_seed(52)) * keep).to(gpu)
    torch.manual_seed(77)
    out = layer(g, feat)
    out.backward(gout)
    got = [out.detach(), feat.grad] + [p.grad for p in (layer.fc.weight, layer.attn_l,
                                                        layer.attn_r, layer.bias)]

    w, al, ar, b = (p.detach().clone().requires_grad_(True)
                    for p in (layer.fc.weight, layer.attn_l, layer.attn_r, layer.bias))
    f2 = feat.detach().clone().requires_grad_(True)
    torch.manual_seed(77)
    h = torch.nn.functional.linear(f2, w)
    el, er = (h * al).sum(-1), (h * ar).sum(-1)
    e = torch.nn.functional.leaky_relu(el[g.idx] + er[g.edge_rows()], 0.2)
    alpha = mk.edge_softmax(g, e)
    unit = g.with_values("sum")
    if nonlinear == "relu":
        x = torch.nn.functional.dropout(h, 0.5, True) if train else h
        rst = mk.dense_aggregate(x, unit, alpha)
    else:
        rst = mk.maxk_aggregate(h, unit, K_L, "exact", dropout_p=0.5 if train else 0.0,
                                training=train, edge_weight=alpha)
    rst = rst + b
    rst.backward(gout)
    want = [rst.detach(), f2.grad, w.grad, al.grad, ar.grad, b.grad]
    for name, a, c in zip(("out", "feat", "fc.weight", "attn_l", "attn_r", "bias"), got, want):
        assert a is not None and float(a.abs().sum()) > 0, name
        assert_same_bits(a.cpu().numpy().reshape(-1), c.cpu().numpy().reshape(-1),
                         f"{nonlinear} train={train}: {name}")
    assert out.shape == (N_L, D_L)


def test_gat_layer_refusals(gpu):
    class DGLLike:
        def adj_tensors(self, fmt):
            raise AssertionError("not reached")

    layer = mk.MaxKGATConv(D_L, D_L, maxk=K_L).to(gpu)
    with pytest.raises(TypeError, match="CSRGraph"):
        layer(DGLLike(), torch.zeros(4, D_L, device=gpu))
    ptr = torch.tensor([0, 1, 1, 2], dtype=torch.int32, device=gpu)
    idx = torch.tensor([1, 0], dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="zero in-degree"):
        layer(mk.CSRGraph(ptr, idx), torch.zeros(3, D_L, device=gpu))
    with pytest.raises(ValueError, match="nonlinear"):
        mk.MaxKGATConv(D_L, D_L, nonlinear="gelu")
    # dglnn.GATConv's initialisation: xavier_normal_ at the relu gain, no bias in fc
    assert layer.fc.bias is None and layer.attn_l.shape == layer.attn_r.shape == (1, D_L)
    assert float(layer.bias.detach().abs().sum()) == 0


def _g(n):
    """gamma(n) = n u / (1 - n u), u = 2^-24: bounds an f32 sum of n products in any order."""
    return n * 2.0 ** -24 / (1 - n * 2.0 ** -24)


@pytest.mark.parametrize("nonlinear", ["maxk", "relu"])
def test_gat_layer_against_a_dense_float64_restatement(gpu, nonlinear):
    """Eval mode, attn_drop = 0. The restatement is dense float64 from the layer's f32 inputs
    and parameters; its two selections come from the layer's own f32 values, never from float64:
    the MaxK mask from torch.topk of the f32 h, the leaky_relu branch s in {1, slope} from the
    sign of the f32 score (so e = s z is linear in both computations). |X| is elementwise, E_X
    the bound on |f32 X - exact X|, u = 2^-24, g(n) = gamma(n), r / c an edge's row / column,
    N nodes, D features, K = k (maxk) or D (relu) terms of an edge's SDDMM sum; dI / dO the
    largest in- / out-degree. Every line is one f32 step of the layer and the bound it adds.

    Forward.
      h = feat W^T          GEMM, inner size D:   E_h = g(D + 3) |feat| |W|^T
      el = sum_f h al       D products:           E_el = E_h |al| + g(D + 3) (|h| + E_h) |al|
      z = el[c] + er[r]     one add:              E_z = (E_el[c] + E_er[r]) (1 + u) + u |z|
      e = s z               one product:          E_e = E_z + u (|e| + E_z)
      alpha = softmax(e)    the kernel is within eps_f = (2 R + ceil(n / 64) + 20) u (+ 2^-126,
                            forward bound above) of the exact softmax of ITS logits, whose range
                            is at most R + 2 D_r, D_r = max E_e of the row; moving every logit of
                            a row by at most D_r moves its softmax by a factor within
                            exp(+-2 D_r):  E_alpha = alpha ((1 + eps_f) exp(2 D_r) - 1) + 2^-125
      x = mask h            exact:                E_x = mask E_h
      agg = A x             a row has <= dI terms: E_agg = g(dI + 3) (A + E_A) (|x| + E_x)
                                                          + E_A (|x| + E_x) + A E_x
      out = agg + b         one add:              E_out = E_agg (1 + u) + u |out|
    Backward from the upstream G (exact).
      b.grad = sum_v G      N terms:              g(N) sum |G|
      ga[e] = <x[c], G[r]>  SDDMM, K terms:       E_ga = g(K + 2) (|x| + E_x)[c] . |G|[r]
                                                         + E_x[c] . |G|[r]
      gh1 = mask A^T G      SSpMM, <= dO terms:   E_gh1 = g(dO + 3) (A + E_A)^T |G| + E_A^T |G|
      ge = alpha (ga - t),  t = sum alpha ga: the kernel is within the backward bound above of
                            the exact value at its own inputs, taken at their upper bounds
                            a+ = alpha + E_alpha, g+ = |ga| + E_ga:
                              B = (ceil(n / 64) + 10) u a+ (g+ + sum a+ g+) + 2^-126
                            and the exact value moves by d alpha (ga - t) + alpha^ (d ga - d t):
                              E_t = sum (E_alpha g+ + alpha E_ga)
                              E_ge = B + E_alpha (|ga| + |t|) + a+ (E_ga + E_t)
      gz = s ge             one product:          E_gz = s E_ge + u (|gz| + s E_ge)
      gel[u] = sum_{c = u} gz, ger[v] = sum_{r = v} gz   (<= dO, dI terms):
                                                  E_gel = g(dO) sum (|gz| + E_gz) + sum E_gz
      gh2 = gel al (gh3 = ger ar), one product:   E_gh2 = E_gel |al| + u (|gel| + E_gel) |al|
      al.grad = sum_u gel h   N products:         g(N + 3) (|gel| + E_gel)^T (|h| + E_h)
                                                  + E_gel^T (|h| + E_h) + |gel|^T E_h
      gh = gh1 + gh2 + gh3  two adds:             E_gh = (1 + g(2)) sum E_ghi + g(2) sum |ghi|
      feat.grad = gh W      GEMM, inner D:        g(D + 3) (|gh| + E_gh) |W| + E_gh |W|
      W.grad = gh^T feat    GEMM, inner N:        g(N + 3) (|gh| + E_gh)^T |feat| + E_gh^T |feat|
    The float64 restatement's own rounding (2^-53 per step) is below 2^-29 of every term."""
    g = _gat_graph(gpu)
    layer = _gat_layer(gpu, nonlinear, False)
    feat = _randn(gpu, (N_L, D_L), 61).requires_grad_(True)
    G32 = _randn(gpu, (N_L, D_L), 62)
    out = layer(g, feat)
    out.backward(G32)
    n, d, u = N_L, D_L, 2.0 ** -24
    K = K_L if nonlinear == "maxk" else d
    r, c = g.edge_rows(), g.idx.long()
    dI, dO = int(g.in_degrees().max()), int(g.out_degrees().max())
    nb = (-(-g.in_degrees() // 64)).double()[r]                      # ceil(n / 64) per edge
    slope = layer.negative_slope

    with torch.no_grad():                                            # the two selections, in f32
        h32 = layer.fc(feat)
        mask = (torch.zeros_like(h32).scatter_(1, h32.topk(K_L, dim=1).indices, 1.0)
                if nonlinear == "maxk" else torch.ones_like(h32)).double()
        z32 = (h32 * layer.attn_l).sum(-1)[g.idx] + (h32 * layer.attn_r).sum(-1)[r]
        s = torch.where(z32 > 0, 1.0, slope).double()

    f, W, al, ar, b = (t.detach().double().requires_grad_(True)
                       for t in (feat, layer.fc.weight, layer.attn_l, layer.attn_r, layer.bias))
    G = G32.double()

    def seg_sum(v):
        return torch.zeros(n, dtype=torch.float64, device=gpu).index_add_(0, r, v)

    def seg_max(v):
        return torch.full((n,), -1e300, dtype=torch.float64, device=gpu).scatter_reduce(
            0, r, v, "amax")

    def dense(v):
        return torch.zeros((n, n), dtype=torch.float64, device=gpu).index_put((r, c), v,
                                                                               accumulate=True)

    h = f @ W.T
    x = h * mask
    el, er = (h * al).sum(-1), (h * ar).sum(-1)
    z = el[c] + er[r]
    e = z * s
    p = (e - seg_max(e.detach())[r]).exp()
    alpha = p / seg_sum(p)[r]
    agg = dense(alpha) @ x
    ref = agg + b
    for t in (h, x, el, er, z, e, alpha):
        t.retain_grad()
    ref.backward(G)

    with torch.no_grad():
        a_ = torch.abs
        # ---- forward
        E_h = _g(d + 3) * (a_(f) @ a_(W).T)
        E_el = (E_h * a_(al)).sum(-1) + _g(d + 3) * ((a_(h) + E_h) * a_(al)).sum(-1)
        E_er = (E_h * a_(ar)).sum(-1) + _g(d + 3) * ((a_(h) + E_h) * a_(ar)).sum(-1)
        E_z = (E_el[c] + E_er[r]) * (1 + u) + u * a_(z)
        E_e = E_z + u * (a_(e) + E_z)
        D_r = seg_max(E_e)[r]
        R = (seg_max(e) + seg_max(-e))[r] + 2 * D_r
        eps_f = (2 * R + nb + 20) * u
        E_alpha = alpha * ((1 + eps_f) * torch.exp(2 * D_r) - 1) + 2.0 ** -125
        E_x = mask * E_h
        A, E_A = dense(alpha), dense(E_alpha)
        xp = a_(x) + E_x
        E_agg = _g(dI + 3) * ((A + E_A) @ xp) + E_A @ xp + A @ E_x
        E_out = E_agg * (1 + u) + u * a_(ref)
        # ---- backward
        aG = a_(G)
        E_b = _g(n) * aG.sum(0)
        ga = alpha.grad
        E_ga = _g(K + 2) * (xp[c] * aG[r]).sum(-1) + (E_x[c] * aG[r]).sum(-1)
        E_gh1 = mask * (_g(dO + 3) * ((A + E_A).T @ aG) + E_A.T @ aG)
        ap, gp = alpha + E_alpha, a_(ga) + E_ga
        B = (nb + 10) * u * ap * (gp + seg_sum(ap * gp)[r]) + 2.0 ** -126
        t = seg_sum(alpha * ga)[r]
        E_t = seg_sum(E_alpha * gp + alpha * E_ga)[r]
        E_ge = B + E_alpha * (a_(ga) + a_(t)) + ap * (E_ga + E_t)
        gz = z.grad
        E_gz = s * E_ge + u * (a_(gz) + s * E_ge)

        def col_sum(v):
            return torch.zeros(n, dtype=torch.float64, device=gpu).index_add_(0, c, v)

        gel, ger = el.grad, er.grad
        E_gel = _g(dO) * col_sum(a_(gz) + E_gz) + col_sum(E_gz)
        E_ger = _g(dI) * seg_sum(a_(gz) + E_gz) + seg_sum(E_gz)
        hp = a_(h) + E_h
        E_al = (_g(n + 3) * ((a_(gel) + E_gel) @ hp) + E_gel @ hp + a_(gel) @ E_h)[None, :]
        E_ar = (_g(n + 3) * ((a_(ger) + E_ger) @ hp) + E_ger @ hp + a_(ger) @ E_h)[None, :]
        gh1 = x.grad * mask
        gh2, gh3 = gel[:, None] * al, ger[:, None] * ar
        E_gh2 = E_gel[:, None] * a_(al) + u * (a_(gel) + E_gel)[:, None] * a_(al)
        E_gh3 = E_ger[:, None] * a_(ar) + u * (a_(ger) + E_ger)[:, None] * a_(ar)
        E_gh = (1 + _g(2)) * (E_gh1 + E_gh2 + E_gh3) + _g(2) * (a_(gh1) + a_(gh2) + a_(gh3))
        assert float((gh1 + gh2 + gh3 - h.grad).abs().max()) <= 1e-12 * float(h.grad.abs().max())
        ghp = a_(h.grad) + E_gh
        E_feat = _g(d + 3) * (ghp @ a_(W)) + E_gh @ a_(W)
        E_W = _g(n + 3) * (ghp.T @ a_(f)) + E_gh.T @ a_(f)

    checks = [("out", out.detach(), ref.detach(), E_out), ("feat", feat.grad, f.grad, E_feat),
              ("fc.weight", layer.fc.weight.grad, W.grad, E_W),
              ("attn_l", layer.attn_l.grad, al.grad, E_al),
              ("attn_r", layer.attn_r.grad, ar.grad, E_ar), ("bias", layer.bias.grad, b.grad, E_b)]
    for name, got, want, bound in checks:
        err = (got.double() - want).abs()
        ratio = float((err / bound).max())
        print(f"\nMaxKGATConv {nonlinear} {name}: worst error / bound {ratio:.3f}, "
              f"bound / |value| median {float((bound / want.abs().clamp(min=1e-30)).median()):.2e}")
        assert float(want.abs().sum()) > 0 and ratio <= 1.0, (name, ratio)
