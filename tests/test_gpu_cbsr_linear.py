"""GPU: the CBSR-times-table kernels (include/maxk_hip.h, "MaxK linear layers") against the float64
restatements of tests/cbsr_linear.py, NaN-filled outputs and dirty scratch throughout; one captured
replay, both Functions against float64 autograd, the layers with and without sparse_linear, and the
closure over the maxk_lin:: fixture. Worst error / bound figures print with -s."""
import os

import numpy as np
import pytest
import torch

import cbsr_linear as cl
import gat_heads as gh
import maxk_kernels as mk
from maxk_kernels import ops

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "kernel_instantiations_linear.txt")
COVERED = set()      # kernel names launched by a case that went on to pass


def strided(t, extra):
    buf = torch.full((t.shape[0], t.shape[1] + extra), 77, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def launch(v, s, T, g, bias, d, pad=0):
    """The three products into NaN-filled outputs with a dirty scratch; pad: extra elements per
    row of every 2-D output."""
    dev, (n, k), m = v.device, v.shape, T.shape[1]
    def dirty(op):
        return torch.full((ops.cbsr_linear_scratch_bytes(op, n, d, k, m),), 0xFF,
                          dtype=torch.uint8, device=dev)
    out_a = ops.cbsr_matmul(v, s, T, bias, out=nan(dev, n, m + pad)[:, :m])
    out_b = ops.cbsr_sampled_matmul(g, s, T, out=nan(dev, n, k + pad)[:, :k],
                                    scratch=dirty(cl.SAMPLED))
    dT, dsum = ops.cbsr_weight_grad(v, s, g, d, with_sum=True,
                                    out=(nan(dev, d, m + pad)[:, :m], nan(dev, d)),
                                    scratch=dirty(cl.WEIGHT_GRAD))
    return out_a, out_b, dT, dsum


VARIANTS = [(c, kind) for c in cl.CASES for kind in ("exact", "real")] + \
    [(cl.CASES[9], "strided"), (cl.CASES[3], "repeat"), (cl.CASES[5], "repeat")]


@pytest.mark.parametrize("shape,kind", VARIANTS)
def test_products_against_float64(gpu, shape, kind):
    n, d, k, m = shape
    exact = kind != "real"
    host = cl.inputs(n, d, k, m, seed=n + d + k + m, exact=exact, repeat=kind == "repeat")
    v, s, T, g, bias = host
    dev = [torch.from_numpy(a).to(gpu) for a in host]
    pad = 0
    if kind == "strided":
        dev[:4] = [strided(t, e) for t, e in zip(dev[:4], (3, 5, 4, 8))]
        assert not any(t.is_contiguous() for t in dev[:4])
        pad = 4
    got = [t.cpu().numpy() for t in launch(*dev, d, pad)]
    out_a, mag_a = cl.matmul64(v, s, T, bias)
    out_b, mag_b = cl.sampled64(g, s, T)
    dT, dsum, mag_t, mag_s, count = cl.weight_grad64(v, s, g, d)
    want = (out_a, out_b, dT, dsum)
    mags = (mag_a, mag_b, mag_t, mag_s)
    terms = (k, m, count[:, None], count)
    for name, a, w, mag, t in zip(("matmul", "sampled", "grad_table", "grad_sum"), got, want, mags,
                                  terms):
        if exact:
            # every partial sum is a multiple of the quantum below 2^24 quanta: exact in any order
            assert mag.max() < 2 ** 24 * cl.QUANTUM
            assert np.array_equal(a, w.astype(np.float32)), (name, shape, kind)
        else:
            ratio = cl.worst(a, w, mag, t)
            print(f"\n{shape} {name}: worst error / bound {ratio:.3f}")
            assert ratio <= 1.0, (name, shape)
    COVERED.update(cl.kernels(d, m))


def test_one_captured_replay_equals_eager(gpu):
    n, d, k, m = 257, 256, 16, 260
    ins = [torch.from_numpy(a).to(gpu) for a in cl.inputs(n, d, k, m, 5, exact=True)]
    static = [t.clone() for t in ins]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        launch(*static, d)  # warm up: code objects loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = launch(*static, d)
    fresh = [torch.roll(t, 1, 0) for t in ins]
    for s_, f in zip(static, fresh):
        s_.copy_(f)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(outs, launch(*fresh, d)):
        assert torch.equal(got, want)


def within(got, want, mag, terms, what):
    ratio = cl.worst(got.detach().cpu().numpy(), want.numpy(), mag.numpy(), terms)
    print(f"\n{what}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, what


GRAD_SHAPE = (257, 64, 8, 100)


def test_cbsr_linear_gradients_against_float64_autograd(gpu):
    n, d, k, m = GRAD_SHAPE
    v, s, T, g, bias = (torch.from_numpy(a) for a in cl.inputs(n, d, k, m, 9, exact=False))
    leaves = [t.to(gpu).requires_grad_(True) for t in (v, T.t().contiguous(), bias)]
    out = mk.cbsr_linear(leaves[0], s.to(gpu), leaves[1], leaves[2])
    (out * g.to(gpu)).sum().backward()
    v64, w64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in leaves)
    idx = s.long()
    def dense(values):
        return torch.zeros(n, d, dtype=torch.float64).scatter_add(1, idx, values)
    ref = dense(v64) @ w64.t() + b64
    (ref * g.double()).sum().backward()
    within(out, ref.detach(), dense(v.abs().double()) @ w64.detach().abs().t() + b64.detach().abs(),
           k, "cbsr_linear")
    count = torch.bincount(idx.reshape(-1), minlength=d).double()
    within(leaves[0].grad, v64.grad, (g.abs().double() @ T.abs().double().t()).gather(1, idx), m,
           "grad sp_data")
    within(leaves[1].grad, w64.grad, g.abs().double().t() @ dense(v.abs().double()),
           count[None, :].numpy(), "grad weight")
    within(leaves[2].grad, b64.grad, g.abs().double().sum(0), n, "grad bias")
    COVERED.update(cl.kernels(d, m))


def test_linear_maxk_gradients_against_float64_autograd(gpu):
    n, d_in, k, d = GRAD_SHAPE[0], GRAD_SHAPE[3], GRAD_SHAPE[2], GRAD_SHAPE[1]
    rng = torch.Generator().manual_seed(4)
    h, w, b, gsp = (torch.randn(shape, generator=rng)
                    for shape in ((n, d_in), (d, d_in), (d,), (n, k)))
    leaves = [t.to(gpu).requires_grad_(True) for t in (h, w, b)]
    sp_data, sp_index = mk.linear_maxk(*leaves, k)
    want_data, want_index = mk.maxk(torch.nn.functional.linear(*leaves), k)
    assert torch.equal(sp_index, want_index) and torch.equal(sp_data, want_data)
    (sp_data * gsp.to(gpu)).sum().backward()
    h64, w64, b64 = (t.double().requires_grad_(True) for t in (h, w, b))
    idx = sp_index.long().cpu()
    ((h64 @ w64.t() + b64).gather(1, idx) * gsp.double()).sum().backward()
    mag = torch.zeros(n, d, dtype=torch.float64).scatter_add(1, idx, gsp.abs().double())
    count = torch.bincount(idx.reshape(-1), minlength=d).double().numpy()
    within(leaves[0].grad, h64.grad, mag @ w.abs().double(), k, "grad h")
    within(leaves[1].grad, w64.grad, mag.t() @ h.abs().double(), count[:, None], "grad weight")
    within(leaves[2].grad, b64.grad, mag.sum(0), count, "grad bias")
    COVERED.update(cl.kernels(d, d_in))


def close(got, want, what):
    rel = float((got.detach().double() - want.detach().double()).norm() / want.detach().norm())
    print(f"\n{what}: relative difference {rel:.2e}")
    assert rel <= 1e-5, what


@pytest.mark.parametrize("kind", ["sage", "gcn"])
def test_layers_with_sparse_linear_match_the_dense_path(gpu, kind):
    ptr, idx = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in gh.graph_arrays())
    graph = mk.CSRGraph(ptr, idx)
    def make(sparse):
        torch.manual_seed(3)
        if kind == "gcn":
            return mk.MaxKGCNConv(40, 64, maxk=16, allow_zero_in_degree=True,
                                  sparse_linear=sparse).to(gpu)
        return mk.MaxKSAGEConv(64, 48, "mean", maxk=16, sparse_linear=sparse).to(gpu)
    results = []
    for sparse in (False, True):
        layer = make(sparse)
        feat = torch.randn(gh.NUM, layer.in_feats, device=gpu,
                           generator=torch.Generator(gpu).manual_seed(8)).requires_grad_(True)
        out = layer(graph, feat)
        (out * torch.randn(out.shape, device=gpu,
                           generator=torch.Generator(gpu).manual_seed(9))).sum().backward()
        results.append([out, feat.grad] + [p.grad for _, p in sorted(layer.named_parameters())])
    names = ["out", "grad feat"] + sorted(n for n, _ in make(True).named_parameters())
    for name, got, want in zip(names, results[1], results[0]):
        close(got, want, f"{kind} {name}")


# ------------------------------------------------------------------ closure (keep last)
def test_every_linear_instantiation_was_launched_by_a_passing_case(gpu):
    names = set(open(FIXTURE).read().split())  # held to the library by test_cbsr_linear_capi.py
    assert len(names) == 8
    missing = sorted(names - COVERED)
    assert not missing, f"instantiations without a passing case: {missing}"
    assert not COVERED - names
