"""GPU: the 16-bit weight gradient on the matrix cores (maxk_cbsr_weight_grad_16, include/maxk_hip.h)
against the float64 sum over the rounded values and g as they are: bit for bit on eighths and on
rounding ties, within (n + 2) 2^-24 sum |terms| on normal inputs. Worst error / bound figures print
with -s.

Measured on an MI355X, worst error / bound over CASES on normal inputs: 0.26 for bf16 and 0.40 for
f16, both in the shapes with a handful of terms per element; 0.006 at N = 5441."""
import os
import sys

import numpy as np
import pytest
import torch

import maxk_kernels as mk
from maxk_kernels import ops
from oracle import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_list  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
CODE = {torch.bfloat16: 1, torch.float16: 2}
U = 2.0 ** -24
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "kernel_instantiations_weight_grad16.txt")

# (N, D, k, M). N around the MFMA depth of 32 and the chunk of 64; 129: three work-groups, the last
# ragged; 5441 = 64 * 85 + 1 (three panels) and 16385 = 64 * 256 + 1 (one): the row groups at their
# cap, one of which walks two chunks and writes its zeros back in between. D around a feature tile
# and every accumulator height, M around the 16-byte load, both panel widths and three panels,
# k = 1, 16, D and past the 64 slots held in registers.
CASES = [(1, 1, 1, 1), (31, 16, 16, 7), (33, 17, 1, 8), (63, 64, 64, 9), (64, 65, 16, 64),
         (65, 256, 16, 65), (129, 64, 1, 129), (129, 128, 100, 260), (65, 100, 16, 128),
         (200, 256, 256, 8), (5441, 256, 16, 260), (16385, 16, 1, 64)]


def kernel_name(d, m, dt):
    dp = 64 if d <= 64 else 128 if d <= 128 else 256
    return f"maxk_wg16::weight_grad16_kernel<{dp}, {128 if m > 64 else 64}, {CODE[dt]}>"


def eighths(rng, *shape):
    return (rng.integers(-8, 9, shape) / 8).astype(np.float32)


def on_ties(rng, dt, *shape):
    """f32 values on the rounding ties of `dt` and one f32 step to either side, above a last kept
    bit of either parity: nonzero eighths with those low bits set."""
    drop = 16 if dt == torch.bfloat16 else 13
    base = (rng.integers(1, 9, shape) * rng.choice([-1, 1], shape) / 8).astype(np.float32)
    low = (1 << (drop - 1)) + rng.integers(-1, 2, shape) + (rng.integers(0, 2, shape) << drop)
    return (base.view(np.int32) | low.astype(np.int32)).view(np.float32)


def tables(n, d, k, m, seed, kind, dt):
    """(sp_data, sp_index, g as f32): the selectors of a top-k of random rows (distinct, ascending);
    values that are eighths, ties or standard normal and not rounded; g holds values of `dt`."""
    rng = np.random.default_rng(seed)
    index = oracle.maxk(rng.standard_normal((n, d)).astype(np.float32), k)[1]
    if kind == "real":
        data, g = (rng.standard_normal(s).astype(np.float32) for s in ((n, k), (n, m)))
        g = torch.from_numpy(g).to(dt).float().numpy()
    else:
        data = on_ties(rng, dt, n, k) if kind == "ties" else eighths(rng, n, k)
        g = eighths(rng, n, m)
    return data, index, g


def reference(data, index, g, d, dt):
    """float64 (table, sums, bound of the table, bound of the sums) over data.to(dt) and g."""
    vr = torch.from_numpy(data).to(dt).double().numpy()
    sel = index.astype(np.int64)
    a = np.zeros((data.shape[0], d))
    np.put_along_axis(a, sel, vr, 1)
    count = np.bincount(sel.reshape(-1), minlength=d)[:, None]
    g64 = g.astype(np.float64)
    return (a.T @ g64, a.sum(0), (count + 2) * U * (np.abs(a).T @ np.abs(g64)),
            (count[:, 0] + 2) * U * np.abs(a).sum(0))


def launch(gpu, dt, data, index, g, d, pad=0, with_sum=True):
    """Into NaN-filled outputs with a dirty scratch; pad: strided rows, g from an odd boundary."""
    n, k = data.shape
    m = g.shape[1]
    data_t, index_t = torch.from_numpy(data).to(gpu), torch.from_numpy(index).to(gpu)
    g_t = torch.from_numpy(g).to(gpu).to(dt)
    table = torch.full((d, m + pad), float("nan"), device=gpu)
    if pad:
        wide = torch.full((n, m + 3 - m % 2), 77., dtype=dt, device=gpu)
        wide[:, 1:m + 1] = g_t
        g_t = wide[:, 1:m + 1]
        assert g_t.data_ptr() % 4 == 2 and (n == 1 or g_t.stride(0) % 2 == 1)
        data_t = torch.cat([data_t, torch.full((n, pad), 9., device=gpu)], 1)[:, :k]
        index_t = torch.cat([index_t, torch.zeros((n, pad), dtype=torch.uint8, device=gpu)], 1)[:, :k]
    sums = torch.full((d,), float("nan"), device=gpu)
    scratch = torch.full((ops.cbsr_weight_grad_16_scratch_bytes(n, d, k, m) + 16,), 0xFF,
                         dtype=torch.uint8, device=gpu)  # every f32 of it is a NaN
    out = (table[:, :m], sums) if with_sum else table[:, :m]
    ops.cbsr_weight_grad_16(data_t, index_t, g_t, d, with_sum=with_sum, out=out, scratch=scratch)
    assert not pad or table[:, m:].isnan().all()
    return table[:, :m].contiguous().cpu().numpy(), sums.cpu().numpy()


def check(got, want, exact, what):
    for name, x, y, bound in (("table", got[0], want[0], want[2]), ("sums", got[1], want[1], want[3])):
        if exact:
            assert np.array_equal(x.view(np.uint32), (y + 0.0).astype(np.float32).view(np.uint32)), \
                (what, name)
            continue
        err = np.abs(x.astype(np.float64) - y)
        assert (err[bound == 0] == 0).all(), (what, name)
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        print(f"\n{what} {name}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, (what, name)


# pad 5: every 2-D array strided, g on an odd 2-byte boundary
VARIANTS = [(c, kind, 0) for c in CASES for kind in ("exact", "real")] + [(CASES[5], "ties", 0)] + \
    [(c, kind, 5) for c in (CASES[2], CASES[7], CASES[8]) for kind in ("exact", "real")]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,kind,pad", VARIANTS)
def test_tables_against_float64(gpu, dt, shape, kind, pad):
    n, d, k, m = shape
    data, index, g = tables(n, d, k, m, n + d + k + m, kind, dt)
    check(launch(gpu, dt, data, index, g, d, pad), reference(data, index, g, d, dt), kind != "real",
          (dt, shape, kind, pad))


def test_the_cases_launch_every_instantiation_of_the_fixture():
    names = {kernel_name(d, m, dt) for _, d, _, m in CASES for dt in DTYPES}
    assert names | {"maxk_wg16::weight_grad16_reduce_kernel"} == set(kernel_list.read_list(FIXTURE))


@pytest.mark.parametrize("dt", DTYPES)
def test_non_finite_inputs_stay_where_a_dense_product_puts_them(gpu, dt):
    n, d, k, m = 129, 100, 16, 130
    data, index, g = tables(n, d, k, m, 5, "real", dt)
    clean = launch(gpu, dt, data, index, g, d)
    bad = data.copy()
    bad[70, 3] = np.nan
    table, sums = launch(gpu, dt, bad, index, g, d)
    others = np.arange(d) != index[70, 3]
    assert np.isnan(table[~others]).all() and np.isnan(sums[~others]).all()
    assert np.array_equal(table[others].view(np.uint32), clean[0][others].view(np.uint32))
    assert np.array_equal(sums[others].view(np.uint32), clean[1][others].view(np.uint32))
    bad_g = g.copy()
    bad_g[100, 129] = np.nan
    table, sums = launch(gpu, dt, data, index, bad_g, d)
    assert np.isnan(table[:, 129]).all()
    assert np.array_equal(table[:, :129].view(np.uint32), clean[0][:, :129].view(np.uint32))
    assert np.array_equal(sums.view(np.uint32), clean[1].view(np.uint32))


@pytest.mark.parametrize("dt", DTYPES)
def test_repeats_bit_for_bit_without_sums_and_writes_zeros_for_no_rows(gpu, dt):
    n, d, k, m = CASES[10]
    data, index, g = tables(n, d, k, m, 8, "real", dt)
    first, again = launch(gpu, dt, data, index, g, d), launch(gpu, dt, data, index, g, d)
    alone = launch(gpu, dt, data, index, g, d, with_sum=False)
    assert np.array_equal(first[0].view(np.uint32), again[0].view(np.uint32))
    assert np.array_equal(first[1].view(np.uint32), again[1].view(np.uint32))
    assert np.array_equal(first[0].view(np.uint32), alone[0].view(np.uint32)) and np.isnan(alone[1]).all()
    table, sums = launch(gpu, dt, data[:0], index[:0], g[:0], d)
    assert not table.any() and not sums.any() and table.shape == (d, m)


@pytest.mark.parametrize("dt", DTYPES)
def test_one_captured_replay_equals_eager(gpu, dt):
    n, d, k, m = 321, 256, 16, 200
    data, index, g = (torch.from_numpy(a).to(gpu) for a in tables(n, d, k, m, 6, "real", dt))
    ins = [data, index, g.to(dt)]
    static = [t.clone() for t in ins]
    scratch = torch.empty(ops.cbsr_weight_grad_16_scratch_bytes(n, d, k, m), dtype=torch.uint8,
                          device=gpu)
    def run(args):
        return ops.cbsr_weight_grad_16(*args, d, with_sum=True, scratch=scratch)
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
    kept = [o.clone() for o in outs]
    for got, want in zip(kept, run(fresh)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("exact", [True, False])
def test_linear_maxk_gradients_against_float64_autograd(gpu, dt, exact):
    """The composition on the rounded inputs (the gradient of the kept values among them), the
    kernel's own selectors fixed."""
    n, d_in, d, k = 257, 100, 64, 8
    rng = np.random.default_rng(4)
    draw = (lambda *s: eighths(rng, *s)) if exact else \
        (lambda *s: rng.standard_normal(s).astype(np.float32))
    h, w, b, gsp = (torch.from_numpy(draw(*s)).to(dt).float()
                    for s in ((n, d_in), (d, d_in), (d,), (n, k)))
    grads = {}
    for flag in (True, False):
        leaves = [t.to(gpu).to(dt).requires_grad_(True) for t in (h, w, b)]
        sp_data, sp_index = mk.linear_maxk(*leaves, k, fused=True, weight_grad_16=flag)
        (sp_data * gsp.to(gpu)).sum().backward()
        grads[flag] = [leaf.grad for leaf in leaves]
        assert all(g.dtype == dt for g in grads[flag])
    if exact:
        for a, c in zip(grads[True], grads[False]):
            assert torch.equal(a.view(torch.int16), c.view(torch.int16))
    h64, w64, b64 = (t.double().requires_grad_(True) for t in (h, w, b))
    idx = sp_index.long().cpu()
    ((h64 @ w64.t() + b64).gather(1, idx) * gsp.double()).sum().backward()
    mag = torch.zeros(n, d, dtype=torch.float64).scatter_add(1, idx, gsp.abs().double())
    count = torch.bincount(idx.reshape(-1), minlength=d).double()
    step = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11  # one rounding of the f32 result
    for name, got, want, m_, terms in (
            ("grad weight", grads[True][1], w64.grad, mag.t() @ h.abs().double(), count[:, None]),
            ("grad bias", grads[True][2], b64.grad, mag.sum(0), count)):
        if exact:
            assert torch.equal(got.cpu(), want.float().to(dt)), name
            continue
        f32 = (terms + 2) * U * m_
        bound = f32 + step * (want.abs() + f32)
        err = (got.double().cpu() - want).abs()
        ratio = float((err[bound > 0] / bound[bound > 0]).max())
        print(f"\n{name} {dt}: worst error / bound {ratio:.3f}")
        assert (err[bound == 0] == 0).all() and ratio <= 1.0, name


@pytest.mark.parametrize("dt", DTYPES)
def test_gcn_layer_with_the_flag_equals_the_layer_without_on_exact_inputs(gpu, dt):
    """In-degree 3 and eighths: `dt` holds the gradient of a kept value, so no bit changes."""
    num = 200
    ptr = torch.arange(0, 3 * num + 1, 3, dtype=torch.int32, device=gpu)
    idx = ((torch.arange(num)[:, None] + torch.tensor([1, 7, 31])) % num).reshape(-1).int().to(gpu)
    graph = mk.CSRGraph(ptr, idx)
    rng = np.random.default_rng(11)
    weight, feat0, gout = (torch.from_numpy(eighths(rng, *s)).to(gpu)
                           for s in ((40, 64), (num, 40), (num, 64)))
    results = []
    for flag in (False, True):
        layer = mk.MaxKGCNConv(40, 64, norm="none", maxk=16, sparse_linear=True, fused_linear=True,
                               linear_dtype=dt, weight_grad_16=flag).to(gpu)
        with torch.no_grad():
            layer.weight.copy_(weight)
        feat = feat0.clone().requires_grad_(True)
        out = layer(graph, feat)
        (out * gout).sum().backward()
        results.append((out.detach(), layer.bias.grad, feat.grad, layer.weight.grad))
    for a, c in zip(*results):
        assert a.dtype == torch.float32 and torch.equal(a, c) and bool(a.any())
