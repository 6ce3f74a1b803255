"""GPU: CBSR rows times a 16-bit table on the matrix cores (maxk_cbsr_matmul_16, include/maxk_hip.h)
against the float64 sum over the rounded values and the table as they are: bit for bit on eighths
and on rounding ties, within (k + 2) 2^-24 sum |terms| on normal inputs. Worst error / bound
figures print with -s.

Measured on an MI355X, worst error / bound over CASES on normal inputs: 0.120 for bf16 and 0.185 for
f16, both at k = 16; 0.005 on the dense rows of k = D = 256."""
import numpy as np
import pytest
import torch

import maxk_kernels as mk
from maxk_kernels import ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
U = 2.0 ** -24

# (N, D, k, M). A tile is 128 rows: N = 1, one less, one more, two tiles plus one, and 10881 =
# 128 * 85 + 1, where the 85 work-groups a panel of three may have leave one of them a second tile
# (its zeros written back in between). D around a depth step and every depth of the product, k = 1,
# 16, past the 64 slots held in registers and k = D (a dense row: a plain GEMM), M around the
# 8-column store, both panel widths and three panels. Every (DP, MP) of the table is launched.
CASES = [(1, 8, 1, 1), (127, 64, 16, 7), (129, 65, 64, 64), (257, 200, 65, 65),
         (127, 64, 64, 129), (129, 256, 256, 256), (257, 256, 16, 300), (10881, 64, 16, 300),
         (129, 200, 1, 64), (257, 65, 16, 129), (127, 8, 1, 256), (1, 256, 64, 7)]


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
    """(sp_data, sp_index, table as f32): random distinct selectors; values that are eighths, ties
    or standard normal and not rounded; the table holds values of `dt`."""
    rng = np.random.default_rng(seed)
    index = np.argsort(rng.random((n, d)), 1)[:, :k].astype(np.uint8)
    if kind == "real":
        data, table = (rng.standard_normal(s).astype(np.float32) for s in ((n, k), (d, m)))
        table = torch.from_numpy(table).to(dt).float().numpy()
    else:
        data = on_ties(rng, dt, n, k) if kind == "ties" else eighths(rng, n, k)
        table = eighths(rng, d, m)
    return data, index, table


def reference(data, index, table, dt):
    """float64 (product, bound) over data.to(dt) and the table; selectors >= D dropped."""
    d = table.shape[0]
    vr = torch.from_numpy(data).to(dt).double().numpy()
    sel = index.astype(np.int64)
    a = np.zeros((data.shape[0], d + 256))
    np.put_along_axis(a, sel, vr, 1)
    a, t64 = a[:, :d], table.astype(np.float64)
    return a @ t64, (data.shape[1] + 2) * U * (np.abs(a) @ np.abs(t64))


def launch(gpu, dt, data, index, table, out_dtype, pad=0):
    """Into a NaN-filled (pad: 55-filled) output, as f32 numpy. pad: data and index strided, the
    table and out with an odd row stride from an odd element, out inside guard rows and columns."""
    n, k = data.shape
    d, m = table.shape
    data_t, index_t = torch.from_numpy(data).to(gpu), torch.from_numpy(index).to(gpu)
    table_t = torch.from_numpy(table).to(gpu).to(dt)
    if not pad:
        out = torch.full((n, m), float("nan"), dtype=out_dtype, device=gpu)
        assert ops.cbsr_matmul_16(data_t, index_t, table_t, out=out) is out
        return out.float().cpu().numpy()
    width = m + 3 - m % 2
    wide = torch.full((d, width), 77., dtype=dt, device=gpu)
    wide[:, 1:m + 1] = table_t
    data_t = torch.cat([data_t, torch.full((n, pad), 9., device=gpu)], 1)[:, :k]
    index_t = torch.cat([index_t, torch.zeros((n, pad), dtype=torch.uint8, device=gpu)], 1)[:, :k]
    buf = torch.full((n + 2, width), 55., dtype=out_dtype, device=gpu)
    out = buf[:n, 1:m + 1]
    assert out.data_ptr() % (2 * out.element_size()) and out.stride(0) % 2 == 1
    ops.cbsr_matmul_16(data_t, index_t, wide[:, 1:m + 1], out=out)
    assert bool((buf[n:] == 55).all() and (buf[:, 0] == 55).all() and (buf[:, m + 1:] == 55).all())
    return out.float().cpu().numpy()


def bits(x):  # of the f32 of x, a -0.0 of the float64 restatement as the sum's +0.0
    return np.ascontiguousarray(x + 0.0, dtype=np.float32).view(np.uint32)


def rounded(x, dt):  # float64 -> f32 -> dt, as f32
    return torch.from_numpy((x + 0.0).astype(np.float32)).to(dt).float().numpy()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", CASES)
def test_normal_inputs_within_the_bound_and_16_bit_is_the_f32_rounded(gpu, dt, shape):
    data, index, table = tables(*shape, sum(shape), "real", dt)
    want, bound = reference(data, index, table, dt)
    got = launch(gpu, dt, data, index, table, torch.float32)
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"\n{dt} {shape}: worst error / bound {ratio:.3f}")
    assert (err[bound == 0] == 0).all() and ratio <= 1.0
    got16 = launch(gpu, dt, data, index, table, dt)
    assert np.array_equal(bits(got16), bits(torch.from_numpy(got).to(dt).float().numpy()))
    assert np.array_equal(bits(got), bits(launch(gpu, dt, data, index, table, torch.float32)))


# ties: where k sum |terms| stays below 2^7 so that every partial sum is an f32
EXACT = [(c, "eighths", 0) for c in CASES] + [(c, "ties", 0) for c in (CASES[3], CASES[6])] + \
    [(c, kind, 5) for c in (CASES[1], CASES[3], CASES[6]) for kind in ("eighths", "ties")]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,kind,pad", EXACT)
def test_exact_inputs_and_layouts_equal_float64_bit_for_bit(gpu, dt, shape, kind, pad):
    data, index, table = tables(*shape, 1 + sum(shape), kind, dt)
    want = reference(data, index, table, dt)[0]
    assert np.array_equal(bits(launch(gpu, dt, data, index, table, torch.float32, pad)), bits(want))
    assert np.array_equal(bits(launch(gpu, dt, data, index, table, dt, pad)),
                          bits(rounded(want, dt)))


@pytest.mark.parametrize("dt", DTYPES)
def test_contract_edges(gpu, dt):
    n, d, k, m = 130, 100, 16, 130
    data, index, table = tables(n, d, k, m, 5, "eighths", dt)
    clean = launch(gpu, dt, data, index, table, torch.float32)
    rows = np.arange(n)
    # a selector >= D contributes nothing; a repeated one takes one of its values
    odd = index.copy()
    odd[7, 0], odd[5, 3] = 200, odd[5, 2]
    got = launch(gpu, dt, data, odd, table, torch.float32)
    keep = rows != 5
    assert np.array_equal(bits(got[keep]), bits(reference(data, odd, table, dt)[0][keep]))
    assert np.array_equal(bits(got[keep & (rows != 7)]), bits(clean[keep & (rows != 7)]))
    one_of = [clean[5] - data[5, 3] * table[index[5, 3]] + (data[5, j] - data[5, 2]) * table[index[5, 2]]
              for j in (2, 3)]
    assert any(np.array_equal(bits(got[5]), bits(x)) for x in one_of)
    # dense-shaped: a NaN of the table reaches its column in every row, one of a value its row
    bad = table.copy()
    bad[index[0, 0], 129] = np.nan
    got = launch(gpu, dt, data, index, bad, dt)
    assert np.isnan(got[:, 129]).all()
    assert np.array_equal(bits(got[:, :129]), bits(rounded(clean[:, :129], dt)))
    bad = data.copy()
    bad[70, 3] = np.nan
    got = launch(gpu, dt, bad, index, table, torch.float32)
    assert np.isnan(got[70]).all() and np.array_equal(bits(got[rows != 70]), bits(clean[rows != 70]))


@pytest.mark.parametrize("dt", DTYPES)
def test_linear_maxk_input_gradient_is_the_direct_call(gpu, dt):
    n, d_in, d, k = 257, 100, 64, 8
    rng = np.random.default_rng(4)
    h, w, gsp = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(gpu)
                 for s in ((n, d_in), (d, d_in), (n, k)))
    grads = {}
    for flag in (True, False):
        leaves = [t.to(dt).requires_grad_(True) for t in (h, w)]
        sp_data, sp_index = mk.linear_maxk(*leaves, None, k, fused=True, weight_grad_16=True,
                                           input_grad_16=flag)
        (sp_data * gsp).sum().backward()
        grads[flag] = leaves[0].grad
        assert grads[flag].dtype == dt and grads[flag].shape == (n, d_in)
    weight = w.to(dt)
    direct = ops.cbsr_matmul_16(gsp, sp_index, weight)
    assert direct.dtype == dt and torch.equal(grads[True].view(torch.int16), direct.view(torch.int16))
    assert torch.equal(direct, torch.ops.maxk.cbsr_matmul_16(gsp, sp_index, weight))
    old = ops.cbsr_matmul(gsp, sp_index, weight.float()).to(dt)
    assert torch.equal(grads[False].view(torch.int16), old.view(torch.int16))
