"""GPU: the fused linear + MaxK kernel (include/maxk_hip.h, "Fused linear + MaxK") against the
float64 h @ W.T + b of numpy: bit for bit on exactly summable inputs, as a property of every row on
normal ones; strided arrays with the dense row, row isolation under NaN, one captured replay, the
gradients of linear_maxk(fused=True) and the GCN layer with and without fused_linear. Outputs are
NaN-filled before every call. Worst error / bound figures print with -s."""
import numpy as np
import pytest
import torch

import cbsr_linear as cl
import gat_heads as gh
import maxk_kernels as mk
from maxk_kernels import ops
from oracle import oracle

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

# (N, D_in, D, k): N around a wave's 16 rows and a work-group's 64, D_in around the MFMA depth of 4
# and the chunk of 32 (33, 5, 3, 1, 31: rows off a 16-byte boundary), D around a column tile of 16
# and every accumulator width (64, 128, 256), k = 1, 8, 16, D (past 64: the wide emission).
CASES = [(1, 1, 1, 1), (15, 3, 15, 8), (16, 4, 16, 16), (17, 5, 17, 1), (63, 31, 64, 8),
         (64, 32, 65, 16), (65, 33, 100, 100), (257, 100, 128, 8), (64, 260, 129, 16),
         (65, 33, 255, 255), (257, 260, 256, 16)]


def inputs(n, d_in, d, seed, exact, ties=False, bias=True):
    """h [n, d_in], W [d, d_in], bias [d] or None in f32: standard normal, or for `exact` multiples
    of 1/8 in [-1, 1] (terms are multiples of 1/64 and sum below 2^24 of them: any order is exact).
    `ties` repeats every even row of W and entry of bias in the odd one after it."""
    rng = np.random.default_rng(seed)
    def draw(*shape):
        if exact:
            return (rng.integers(-8, 9, shape) / 8).astype(np.float32)
        return rng.standard_normal(shape).astype(np.float32)
    h, w, b = draw(n, d_in), draw(d, d_in), draw(d)
    if ties:
        w[1::2], b[1::2] = w[0::2][:d // 2], b[0::2][:d // 2]
    return h, w, (b if bias else None)


def reference(h, w, b):
    """float64 pre-activation and its bound (n + 2) u sum |terms|, n = D_in (+ 1 with a bias)."""
    y = h.astype(np.float64) @ w.astype(np.float64).T
    mag = np.abs(h).astype(np.float64) @ np.abs(w).astype(np.float64).T
    if b is not None:
        y, mag = y + b.astype(np.float64), mag + np.abs(b).astype(np.float64)
    return y, (h.shape[1] + (b is not None) + 2) * U * mag


def padded(t, extra, fill=float("nan")):
    buf = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf, buf[:, :t.shape[1]]


def launch(gpu, h, w, b, k, pad=0):
    """ops.linear_topk into NaN / 0xAB filled tables; pad > 0: every array row-strided, the dense
    row asked for, and the bytes between rows checked to be untouched. Returns numpy arrays."""
    dev = [None if a is None else torch.from_numpy(a).to(gpu) for a in (h, w, b)]
    n, d = h.shape[0], w.shape[0]
    if pad:
        dev[0], dev[1] = padded(dev[0], 3, 77.)[1], padded(dev[1], 4, 77.)[1]
    data_buf, data = padded(torch.empty(n, k, device=gpu), pad)
    index_buf, index = padded(torch.empty(n, k, dtype=torch.uint8, device=gpu), pad, 0xAB)
    dense_buf, dense = padded(torch.empty(n, d, device=gpu), pad)
    data.fill_(float("nan")), index.fill_(0xAB), dense.fill_(float("nan"))
    ops.linear_topk(dev[0], dev[1], dev[2], k, out=(data, index), dense=dense if pad else None)
    if pad:
        assert not data.is_contiguous() and not dev[0].is_contiguous()
        assert data_buf[:, k:].isnan().all() and dense_buf[:, d:].isnan().all()
        assert (index_buf[:, k:] == 0xAB).all()
        want = torch.zeros(n, d, device=gpu).scatter_(1, index.long(), data)
        assert torch.equal(dense.view(torch.int32), want.view(torch.int32))  # +0.0 elsewhere
    return data.contiguous().cpu().numpy(), index.contiguous().cpu().numpy()


def check(got, h, w, b, k, exact, what):
    data, index = got
    y, bound = reference(h, w, b)
    if exact:
        # + 0.0: the kernel's sum starts from +0.0, so a pre-activation is never -0.0
        want_data, want_index = oracle.maxk((y + 0.0).astype(np.float32), k)
        assert np.array_equal(index, want_index), what
        assert np.array_equal(data.view(np.uint32), want_data.view(np.uint32)), what
        return
    sel = index.astype(np.int64)
    assert (np.diff(sel, axis=1) > 0).all(), what
    err = np.abs(data - np.take_along_axis(y, sel, 1))
    lim = np.take_along_axis(bound, sel, 1)
    ratio = float((err / lim).max())
    print(f"\n{what}: worst error / bound {ratio:.3f}")
    assert np.isfinite(data).all() and ratio <= 1.0, what
    chosen = np.zeros(y.shape, bool)
    np.put_along_axis(chosen, sel, True, 1)
    low = np.where(chosen, y + bound, np.inf).min(1)
    high = np.where(chosen, -np.inf, y - bound).max(1)
    assert (low >= high).all(), what


VARIANTS = [(c, kind, 0) for c in CASES for kind in ("exact", "real")] + \
    [(CASES[8], "ties", 0), (CASES[5], "nobias", 0), (CASES[10], "nobias-real", 0)] + \
    [(c, kind, 4) for c in (CASES[4], CASES[6], CASES[7], CASES[10]) for kind in ("exact", "real")]


@pytest.mark.parametrize("shape,kind,pad", VARIANTS)
def test_tables_against_float64(gpu, shape, kind, pad):
    n, d_in, d, k = shape
    exact = not kind.endswith("real")
    h, w, b = inputs(n, d_in, d, n + d_in + d + k, exact, ties=kind == "ties",
                     bias=not kind.startswith("nobias"))
    check(launch(gpu, h, w, b, k, pad), h, w, b, k, exact, (shape, kind, pad))


def test_a_nan_row_stays_in_its_row(gpu):
    n, d_in, d, k = 65, 33, 100, 8
    h, w, b = inputs(n, d_in, d, 7, exact=False)
    clean = launch(gpu, h, w, b, k)
    h2 = h.copy()
    h2[37] = np.nan
    data, index = launch(gpu, h2, w, b, k)
    want_data, want_index = oracle.maxk(np.full((1, d), np.nan, np.float32), k)
    assert np.array_equal(index[37], want_index[0]) and np.isnan(data[37]).all()
    assert np.isnan(want_data).all()
    others = np.arange(n) != 37
    assert np.array_equal(index[others], clean[1][others])
    assert np.array_equal(data[others].view(np.uint32), clean[0][others].view(np.uint32))


def test_one_captured_replay_equals_eager(gpu):
    n, d_in, d, k = 257, 100, 256, 16
    ins = [torch.from_numpy(a).to(gpu) for a in inputs(n, d_in, d, 5, exact=False)]
    static = [t.clone() for t in ins]
    def run(args):
        dense = torch.full((n, d), float("nan"), device=gpu)
        return ops.linear_topk(*args, k, dense=dense) + (dense,)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run(static)  # warm up: code objects loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(static)
    fresh = [torch.roll(t, 1, 0) for t in ins]
    for s_, f in zip(static, fresh):
        s_.copy_(f)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, run(fresh)):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


def test_fused_linear_maxk_gradients_against_float64_autograd(gpu):
    n, d_in, d, k = 257, 100, 64, 8
    rng = torch.Generator().manual_seed(4)
    h, w, b, gsp = (torch.randn(shape, generator=rng)
                    for shape in ((n, d_in), (d, d_in), (d,), (n, k)))
    leaves = [t.to(gpu).requires_grad_(True) for t in (h, w, b)]
    sp_data, sp_index = mk.linear_maxk(*leaves, k, fused=True)
    check((sp_data.detach().cpu().numpy(), sp_index.cpu().numpy()), h.numpy(), w.numpy(), b.numpy(),
          k, False, "linear_maxk fused forward")
    (sp_data * gsp.to(gpu)).sum().backward()
    h64, w64, b64 = (t.double().requires_grad_(True) for t in (h, w, b))
    idx = sp_index.long().cpu()  # the kernel's own selectors, fixed
    ((h64 @ w64.t() + b64).gather(1, idx) * gsp.double()).sum().backward()
    mag = torch.zeros(n, d, dtype=torch.float64).scatter_add(1, idx, gsp.abs().double())
    count = torch.bincount(idx.reshape(-1), minlength=d).double().numpy()
    for name, got, want, m, terms in (
            ("grad h", leaves[0].grad, h64.grad, mag @ w.abs().double(), k),
            ("grad weight", leaves[1].grad, w64.grad, mag.t() @ h.abs().double(), count[:, None]),
            ("grad bias", leaves[2].grad, b64.grad, mag.sum(0), count)):
        ratio = cl.worst(got.cpu().numpy(), want.numpy(), m.numpy(), terms)
        print(f"\n{name}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, name


def test_gcn_layer_with_fused_linear_equals_the_unfused_one_on_exact_inputs(gpu):
    ptr, idx = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in gh.graph_arrays())
    graph = mk.CSRGraph(ptr, idx)
    rng = np.random.default_rng(11)
    def eighths(*shape):
        return torch.from_numpy((rng.integers(-8, 9, shape) / 8).astype(np.float32)).to(gpu)
    weight, feat0, gout = eighths(40, 64), eighths(gh.NUM, 40), eighths(gh.NUM, 64)
    results = []
    for fused in (False, True):
        # norm="none": edge values of 1, so the aggregation and the weight gradient, whose order of
        # summation is not fixed from call to call, are exact as well
        layer = mk.MaxKGCNConv(40, 64, norm="none", maxk=16, allow_zero_in_degree=True,
                               sparse_linear=True, fused_linear=fused).to(gpu)
        with torch.no_grad():
            layer.weight.copy_(weight)
        feat = feat0.clone().requires_grad_(True)
        out = layer(graph, feat)
        (out * gout).sum().backward()
        results.append((out.detach(), feat.grad, layer.weight.grad, layer.bias.grad))
    for got, want in zip(results[1], results[0]):
        assert torch.equal(got, want)
