"""GPU: the fused linear + MaxK kernel on bf16 / f16 operands (include/maxk_hip.h) against the
float64 product of the rounded inputs, with the helpers and the checks of test_gpu_linear_topk.py:
bit for bit on eighths, the contract with constant 1 and the row property on normal inputs. Worst
error / bound figures print with -s."""
import numpy as np
import pytest
import torch

import gat_heads as gh
import maxk_kernels as mk
from maxk_kernels import ops
from oracle import oracle
from test_gpu_linear_topk import U, check, inputs, padded

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
# one rounding of an f32 result to the type: bf16 keeps 8 significant bits, f16 11
ROUND = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# (N, D_in, D, k): N around a wave's 16 rows and a work-group's 128, D_in around a lane's 8 elements,
# the MFMA depth of 32 and the chunk of 64 (odd: rows on 2-byte boundaries), D around a column tile
# of 16 and every accumulator width (64, 128, 256), k = 1, 8, 16, D (past 64: the wide emission).
CASES = [(1, 1, 1, 1), (15, 7, 16, 8), (16, 9, 17, 16), (17, 31, 64, 1), (127, 33, 65, 16),
         (128, 63, 128, 8), (129, 65, 129, 129), (33, 64, 255, 255), (130, 32, 100, 100),
         (257, 260, 256, 16), (129, 8, 256, 1), (260, 100, 64, 8)]


def rounded(dt, *arrays):
    """The f32 arrays rounded to `dt` and back: what the kernel is given, as the reference reads it"""
    return [torch.from_numpy(a).to(dt).float().numpy() for a in arrays]


def launch(gpu, dt, h, w, b, k, pad=0):
    """ops.linear_topk on `dt` copies of h and w into NaN / 0xAB filled tables; pad > 0: every array
    row-strided (h on 2-byte boundaries), the dense row asked for, nothing written between rows."""
    h16, w16 = (torch.from_numpy(a).to(gpu).to(dt) for a in (h, w))
    bias = None if b is None else torch.from_numpy(b).to(gpu)
    n, d = h.shape[0], w.shape[0]
    if pad:
        hb = torch.full((n, h.shape[1] + 3 - h.shape[1] % 2), 77., dtype=dt, device=gpu)
        hb[:, 1:h.shape[1] + 1] = h16
        h16, w16 = hb[:, 1:h.shape[1] + 1], padded(w16, 4, 77.)[1]
        assert h16.data_ptr() % 4 == 2 and h16.stride(0) % 2 == 1 and not w16.is_contiguous()
    data_buf, data = padded(torch.empty(n, k, device=gpu), pad)
    index_buf, index = padded(torch.empty(n, k, dtype=torch.uint8, device=gpu), pad, 0xAB)
    dense_buf, dense = padded(torch.empty(n, d, device=gpu), pad)
    data.fill_(float("nan")), index.fill_(0xAB), dense.fill_(float("nan"))
    ops.linear_topk(h16, w16, bias, k, out=(data, index), dense=dense if pad else None)
    if pad:
        assert data_buf[:, k:].isnan().all() and dense_buf[:, d:].isnan().all()
        assert (index_buf[:, k:] == 0xAB).all()
        want = torch.zeros(n, d, device=gpu).scatter_(1, index.long(), data)
        assert torch.equal(dense.view(torch.int32), want.view(torch.int32))  # +0.0 elsewhere
    return data.contiguous().cpu().numpy(), index.contiguous().cpu().numpy()


VARIANTS = [(c, kind, 0) for c in CASES for kind in ("exact", "real")] + \
    [(CASES[6], "ties", 0), (CASES[4], "nobias", 0), (CASES[9], "nobias-real", 0)] + \
    [(c, kind, 4) for c in (CASES[3], CASES[5], CASES[6], CASES[9]) for kind in ("exact", "real")]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,kind,pad", VARIANTS)
def test_tables_against_float64(gpu, dt, shape, kind, pad):
    n, d_in, d, k = shape
    exact = not kind.endswith("real")
    h, w, b = inputs(n, d_in, d, n + d_in + d + k, exact, ties=kind == "ties",
                     bias=not kind.startswith("nobias"))
    h, w = rounded(dt, h, w)  # eighths are unchanged
    check(launch(gpu, dt, h, w, b, k, pad), h, w, b, k, exact, (dt, shape, kind, pad))


@pytest.mark.parametrize("dt", DTYPES)
def test_a_nan_row_stays_in_its_row(gpu, dt):
    n, d_in, d, k = 130, 33, 100, 8
    h, w, b = inputs(n, d_in, d, 7, exact=False)
    clean = launch(gpu, dt, h, w, b, k)
    h2 = h.copy()
    h2[37] = np.nan
    data, index = launch(gpu, dt, h2, w, b, k)
    want_index = oracle.maxk(np.full((1, d), np.nan, np.float32), k)[1]
    assert np.array_equal(index[37], want_index[0]) and np.isnan(data[37]).all()
    others = np.arange(n) != 37
    assert np.array_equal(index[others], clean[1][others])
    assert np.array_equal(data[others].view(np.uint32), clean[0][others].view(np.uint32))


@pytest.mark.parametrize("dt", DTYPES)
def test_one_captured_replay_equals_eager(gpu, dt):
    n, d_in, d, k = 257, 100, 256, 16
    h, w, b = (torch.from_numpy(a).to(gpu) for a in inputs(n, d_in, d, 5, exact=False))
    ins = [h.to(dt), w.to(dt), b]
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


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_linear_maxk_gradients_against_float64_autograd(gpu, dt):
    n, d_in, d, k = 257, 100, 64, 8
    rng = torch.Generator().manual_seed(4)
    h, w, b, gsp = (torch.randn(shape, generator=rng)
                    for shape in ((n, d_in), (d, d_in), (d,), (n, k)))
    h, w, b = (t.to(dt).float() for t in (h, w, b))  # the rounded inputs, as f32
    leaves = [t.to(gpu).to(dt).requires_grad_(True) for t in (h, w, b)]
    sp_data, sp_index = mk.linear_maxk(*leaves, k, fused=True)
    assert sp_data.dtype == torch.float32 and sp_index.dtype == torch.uint8
    check((sp_data.detach().cpu().numpy(), sp_index.cpu().numpy()), h.numpy(), w.numpy(), b.numpy(),
          k, False, f"linear_maxk fused forward {dt}")
    (sp_data * gsp.to(gpu)).sum().backward()
    h64, w64, b64 = (t.double().requires_grad_(True) for t in (h, w, b))
    idx = sp_index.long().cpu()  # the kernel's own selectors, fixed
    ((h64 @ w64.t() + b64).gather(1, idx) * gsp.double()).sum().backward()
    mag = torch.zeros(n, d, dtype=torch.float64).scatter_add(1, idx, gsp.abs().double())
    count = torch.bincount(idx.reshape(-1), minlength=d).double()
    for name, leaf, want, m, terms in (
            ("grad h", leaves[0], h64.grad, mag @ w.abs().double(), k),
            ("grad weight", leaves[1], w64.grad, mag.t() @ h.abs().double(), count[:, None]),
            ("grad bias", leaves[2], b64.grad, mag.sum(0), count)):
        assert leaf.grad.dtype == dt, name
        # the f32 kernels' bound (test_gpu_linear_topk.py), then one rounding of that f32 result
        f32 = (terms + 2) * U * m
        bound = f32 + ROUND[dt] * (want.abs() + f32)
        err = (leaf.grad.double().cpu() - want).abs()
        assert (err[bound == 0] == 0).all(), name
        ratio = float((err[bound > 0] / bound[bound > 0]).max())
        print(f"\n{name} {dt}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, name


@pytest.mark.parametrize("dt", DTYPES)
def test_gcn_layer_with_linear_dtype_equals_the_f32_layer_on_exact_inputs(gpu, dt):
    """Eighths: the casts, both products and the aggregation are exact, so the output equals the
    linear_dtype=None layer's bit for bit, and so does the bias gradient. The gradients of feat and
    weight leave linear_maxk in `dt` (autograd gives a 16-bit tensor a 16-bit gradient), so they
    are the f32 layer's gradients rounded once to `dt`, bit for bit, and arrive as f32."""
    ptr, idx = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in gh.graph_arrays())
    graph = mk.CSRGraph(ptr, idx)
    rng = np.random.default_rng(11)
    def eighths(*shape):
        return torch.from_numpy((rng.integers(-8, 9, shape) / 8).astype(np.float32)).to(gpu)
    weight, feat0, gout = eighths(40, 64), eighths(gh.NUM, 40), eighths(gh.NUM, 64)
    results = []
    for linear_dtype in (None, dt):
        layer = mk.MaxKGCNConv(40, 64, norm="none", maxk=16, allow_zero_in_degree=True,
                               sparse_linear=True, fused_linear=True,
                               linear_dtype=linear_dtype).to(gpu)
        with torch.no_grad():
            layer.weight.copy_(weight)
        feat = feat0.clone().requires_grad_(True)
        out = layer(graph, feat)
        (out * gout).sum().backward()
        results.append((out.detach(), layer.bias.grad, feat.grad, layer.weight.grad))
    (out32, bias32, feat32, weight32), got = results
    assert all(g.dtype == torch.float32 for g in got)
    for g, want in zip(got, (out32, bias32, feat32.to(dt).float(), weight32.to(dt).float())):
        assert torch.equal(g, want)
