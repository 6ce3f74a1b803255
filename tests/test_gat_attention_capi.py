"""CPU: the GAT attention entry points (maxk_gat_attention_forward / _backward, maxk_edge_colsum)
are declared, bound, and refuse bad arguments on the host before any device call;
CSRGraph.transposed_order; and the float64 restatement, the sum bounds (include/maxk_hip.h, "GAT
attention") and the test graph that test_gpu_gat_attention.py holds the kernels to."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import maxk_kernels as mk
from maxk_kernels import _lib, ops
from test_edge_softmax_capi import (INVALID, P, U, _declared, _rows, _segment_sum,
                                    softmax_backward_rows64, softmax_rows64)
from test_gpu_edge_softmax import LENGTHS, layout, ptr_of, regime

LIMITS = ops.edge_softmax_row_limits()
REGIMES = len(LIMITS) + 1
F = ctypes.c_float
# the entry points under test, resolved once: the module needs the library that has them
GAT_FWD, GAT_BWD, COLSUM = (getattr(_lib.lib, name) for name in (
    "maxk_gat_attention_forward", "maxk_gat_attention_backward", "maxk_edge_colsum"))


# ------------------------------------------------------------------ the formulas, in float64
def scores64(ptr, idx, el, er):
    """z = el[c] + er[r] per edge, float64 from the f32 vectors."""
    rows = _rows(ptr)[1]
    el = np.asarray(el, np.float32).astype(np.float64)
    er = np.asarray(er, np.float32).astype(np.float64)
    return el[np.asarray(idx, np.int64)] + er[rows]


def leaky(z, slope):
    """z > 0 ? z : z * slope (NaN takes the product branch, as in the kernels and in torch)."""
    with np.errstate(all="ignore"):
        return np.where(z > 0, z, z * np.float64(np.float32(slope)))


def attention64(ptr, idx, el, er, slope):
    """float64 attention weights from f32 el, er: softmax over each row of leaky(z). The scores
    are rounded to f32 first (one add, one product), as the kernel's are, then softmax_rows64."""
    z32 = (np.asarray(el, np.float32)[np.asarray(idx, np.int64)] +
           np.asarray(er, np.float32)[_rows(ptr)[1]])
    with np.errstate(all="ignore"):
        x32 = np.where(z32 > 0, z32, z32 * np.float32(slope)).astype(np.float32)
    return softmax_rows64(ptr, x32)


def row_sums64(ptr, v):
    return _segment_sum(np.asarray(v, np.float64), np.asarray(ptr, np.int64))


def col_sums64(idx, v, num_cols):
    out = np.zeros(num_cols, np.float64)
    np.add.at(out, np.asarray(idx, np.int64), np.asarray(v, np.float64))
    return out


def sum_bound(n, abs_sum):
    """(ceil(n / 64) + 8) u sum |terms|: a sum of n f32 terms through at most ceil(n / 64) + 6
    additions (64 or more accumulators in order, then a balanced tree), two units spare for the
    second-order term."""
    n = np.asarray(n, np.int64)
    return (-(-n // 64) + 8) * U * np.asarray(abs_sum, np.float64)


def row_sum_bound(ptr, v):
    return sum_bound(np.diff(np.asarray(ptr, np.int64)), row_sums64(ptr, np.abs(v)))


def col_sum_bound(idx, v, num_cols):
    n = np.bincount(np.asarray(idx, np.int64), minlength=num_cols)
    return sum_bound(n, col_sums64(idx, np.abs(v), num_cols))


def attention_backward64(ptr, idx, el, er, slope, alpha, grad_alpha, num_cols):
    """(grad_edge, grad_er, grad_el) in float64 from f32 alpha and grad_alpha."""
    ge = softmax_backward_rows64(ptr, alpha, grad_alpha)
    z = scores64(ptr, idx, el, er)
    grad_edge = np.where(z > 0, ge, ge * np.float64(np.float32(slope)))
    return grad_edge, row_sums64(ptr, grad_edge), col_sums64(idx, grad_edge, num_cols)


def transposed(idx, num_cols):
    """(ptr_t int32 [num_cols + 1], order int32 [E]): the CSC pointer and, per CSC position,
    the CSR edge, columns ascending and CSR order kept inside a column."""
    idx = np.asarray(idx, np.int64)
    order = np.argsort(idx, kind="stable").astype(np.int32)
    ptr_t = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=num_cols))])
    return ptr_t.astype(np.int32), order


@functools.lru_cache(maxsize=None)
def graph_arrays():
    """(ptr int32, idx int32) of the test graph: the row degrees of test_gpu_edge_softmax.py's
    layout, and columns running through the same multiset of lengths (column c occurs deg[c]
    times, at fixed shuffled places: repeated (row, column) pairs are ordinary edges)."""
    deg, _ = layout()
    idx = np.repeat(np.arange(deg.size), deg)
    idx = idx[np.random.default_rng(71).permutation(idx.size)].astype(np.int32)
    ptr = ptr_of(deg)
    for a in (ptr, idx):
        a.setflags(write=False)
    return ptr, idx


def test_the_test_graph_covers_every_regime_on_both_sides():
    ptr, idx = graph_arrays()
    n = ptr.size - 1
    for lengths in (np.diff(ptr), np.bincount(idx, minlength=n)):
        have = set(lengths.tolist())
        assert {0, 1, 2, 3} <= have
        for L in LIMITS:
            assert {L - 1, L, L + 1} <= have
            assert regime(L) + 1 == regime(L + 1)
        assert {regime(int(v)) for v in have if v} == set(range(REGIMES))
        assert max(have) > 2 * max(LIMITS) and have == set(LENGTHS)
    assert sorted(np.diff(ptr).tolist()) != np.diff(ptr).tolist()
    assert np.bincount(idx, minlength=n).tolist() == np.diff(ptr).tolist()


def test_restatement_against_torch_autograd_in_float64():
    rng = np.random.default_rng(3)
    n, c = 9, 7
    deg = rng.integers(0, 6, n)
    deg[2] = 0
    ptr = ptr_of(deg)
    e = int(ptr[-1])
    idx = rng.integers(0, c, e).astype(np.int32)
    el = rng.standard_normal(c).astype(np.float32)
    er = rng.standard_normal(n).astype(np.float32)
    w = rng.standard_normal(e).astype(np.float32)
    rows = torch.from_numpy(_rows(ptr)[1])
    for slope in (0.2, 0.0, 1.0):
        tl = torch.from_numpy(el).double().requires_grad_(True)
        tr = torch.from_numpy(er).double().requires_grad_(True)
        z = tl[torch.from_numpy(idx).long()] + tr[rows]
        x = torch.nn.functional.leaky_relu(z, float(np.float32(slope)))
        assert np.array_equal(z.detach().numpy(), scores64(ptr, idx, el, er))
        assert np.array_equal(x.detach().numpy(), leaky(z.detach().numpy(), slope))
        alpha = torch.cat([torch.softmax(x[ptr[r]:ptr[r + 1]], 0) for r in range(n)])
        alpha.retain_grad()
        (alpha * torch.from_numpy(w).double()).sum().backward()
        a64 = attention64(ptr, idx, el, er, slope)
        np.testing.assert_allclose(a64, alpha.detach().numpy(), rtol=1e-6, atol=1e-9)
        a32 = alpha.detach().numpy().astype(np.float32)
        ge, ger, gel = attention_backward64(ptr, idx, el, er, slope, a32, w, c)
        np.testing.assert_allclose(ger, tr.grad.numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(gel, tl.grad.numpy(), rtol=1e-5, atol=1e-7)
        assert ger[2] == 0 and np.array_equal(row_sums64(ptr, ge), ger)


def test_sum_bounds_on_hand_rows():
    assert sum_bound(0, 0.0) == 0 and sum_bound(1, 2.0) == 9 * U * 2
    assert sum_bound(64, 1.0) == 9 * U and sum_bound(65, 1.0) == 10 * U
    assert sum_bound(5000, 1.0) == (79 + 8) * U
    b = row_sum_bound([0, 2, 2, 3], [1.0, -3.0, 0.5])
    assert b.tolist() == [9 * U * 4, 0.0, 9 * U * 0.5]
    b = col_sum_bound([1, 1, 0], [1.0, -3.0, 0.5], 3)
    assert b.tolist() == [9 * U * 0.5, 9 * U * 4, 0.0]
    pt, order = transposed([2, 0, 2, 1], 4)
    assert pt.tolist() == [0, 1, 2, 4, 4] and order.tolist() == [1, 3, 0, 2]
    # an f32 implementation in the kernels' placement stays well inside the bound
    rng = np.random.default_rng(5)
    for n in (1, 63, 65, 1025, 5000):
        v = rng.standard_normal(n).astype(np.float32)
        acc = np.zeros(64, np.float32)
        for i in range(0, n, 64):
            acc[:min(64, n - i)] += v[i:i + 64]
        while acc.size > 1:
            acc = acc[0::2] + acc[1::2]
        assert abs(float(acc[0]) - v.astype(np.float64).sum()) <= \
            sum_bound(n, np.abs(v.astype(np.float64)).sum()) / 3


# ------------------------------------------------------------------ CSRGraph.transposed_order
def test_transposed_order_is_the_int32_copy_and_is_cached():
    ptr, idx = graph_arrays()
    g = mk.CSRGraph(torch.from_numpy(ptr.copy()), torch.from_numpy(idx.copy()))
    st = g.transposed_structure()
    order = g.transposed_order()
    assert order.dtype == torch.int32 and order.is_contiguous()
    assert torch.equal(order.long(), st[2]) and st[2].dtype == torch.int64
    assert g.transposed_order() is order
    assert g.transposed_structure() is st and len(st) == 3
    pt, o2 = transposed(idx, ptr.size - 1)
    assert np.array_equal(st[0].numpy(), pt) and np.array_equal(order.numpy(), o2)


# ------------------------------------------------------------------ the C entry points
I32, I64 = ctypes.c_int32, ctypes.c_int64
FWD_ARGS = [P, P, P, P, F, P, I32, I32, I64, P]
BWD_ARGS = [P, P, P, P, F, P, P, P, P, I32, I32, I64, P]
COL_ARGS = [P, P, P, P, I32, I64, P]


def test_header_declares_and_binding_binds_the_entry_points():
    ci, cf, f_ = "const int32_t*", "const float*", "float*"
    assert _declared("maxk_gat_attention_forward") == [
        ci, ci, cf, cf, "float", f_, "int32_t", "int32_t", "int64_t", "void*"]
    assert _declared("maxk_gat_attention_backward") == [
        ci, ci, cf, cf, "float", cf, cf, f_, f_, "int32_t", "int32_t", "int64_t", "void*"]
    assert _declared("maxk_edge_colsum") == [ci, ci, cf, f_, "int32_t", "int64_t", "void*"]
    for name, args in [("maxk_gat_attention_forward", FWD_ARGS),
                       ("maxk_gat_attention_backward", BWD_ARGS),
                       ("maxk_edge_colsum", COL_ARGS)]:
        res, sig = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and sig == args
        assert getattr(_lib.lib, name).argtypes == args
    assert _lib.lib.maxk_abi_version() == 4      # new symbols only


B = 1 << 24   # fake device addresses, far apart: nothing is dereferenced on the host
# the default call: num_rows 10, num_cols 12, 100 edges
SIZES = dict(ptr=44, idx=400, el=48, er=40, alpha=400, grad_alpha=400, grad_edge=400, grad_er=40,
             ptr_t=52, order=400, values=400, out=48)


def _fwd(ptr=P(B), idx=P(2 * B), el=P(3 * B), er=P(4 * B), slope=0.2, alpha=P(5 * B), n=10, c=12,
         e=100):
    rc = GAT_FWD(ptr, idx, el, er, slope, alpha, n, c, e, None)
    return rc, _lib.lib.maxk_last_error().decode()


def _bwd(ptr=P(B), idx=P(2 * B), el=P(3 * B), er=P(4 * B), slope=0.2, alpha=P(5 * B),
         grad_alpha=P(6 * B), grad_edge=P(7 * B), grad_er=P(8 * B), n=10, c=12, e=100):
    rc = GAT_BWD(ptr, idx, el, er, slope, alpha, grad_alpha, grad_edge, grad_er, n, c, e, None)
    return rc, _lib.lib.maxk_last_error().decode()


def _col(ptr_t=P(B), order=P(2 * B), values=P(3 * B), out=P(4 * B), c=12, e=100):
    rc = COLSUM(ptr_t, order, values, out, c, e, None)
    return rc, _lib.lib.maxk_last_error().decode()


FWD_PTRS = ("ptr", "idx", "el", "er", "alpha")
BWD_PTRS = ("ptr", "idx", "el", "er", "alpha", "grad_alpha", "grad_edge", "grad_er")
COL_PTRS = ("ptr_t", "order", "values", "out")
NAME = {_fwd: "maxk_gat_attention_forward", _bwd: "maxk_gat_attention_backward",
        _col: "maxk_edge_colsum"}


@pytest.mark.parametrize("call,which", [(_fwd, w) for w in FWD_PTRS] +
                         [(_bwd, w) for w in BWD_PTRS] + [(_col, w) for w in COL_PTRS])
def test_null_pointers_are_refused(call, which):
    rc, msg = call(**{which: None})
    assert rc == INVALID and NAME[call] in msg and "null pointer" in msg


def test_zero_size_calls_launch_nothing():
    none_f = {k: None for k in FWD_PTRS}
    none_b = {k: None for k in BWD_PTRS}
    none_c = {k: None for k in COL_PTRS}
    for n, c, e in [(0, 0, 0), (0, 12, 0), (0, 12, 5), (0, 0, 5)]:
        assert _fwd(n=n, c=c, e=e, **none_f)[0] == 0
        assert _bwd(n=n, c=c, e=e, **none_b)[0] == 0
    assert _fwd(n=10, c=12, e=0, **none_f)[0] == 0     # alpha has no element
    for e in (0, 5):
        assert _col(c=0, e=e, **none_c)[0] == 0


BAD_SIZES = [dict(c=-1), dict(e=-1), dict(e=2 ** 31), dict(e=2 ** 40)]


@pytest.mark.parametrize("call,kw", [(f, kw) for f in (_fwd, _bwd, _col) for kw in BAD_SIZES] +
                         [(_fwd, dict(n=-1)), (_bwd, dict(n=-1))])
def test_sizes_out_of_range_are_refused(call, kw):
    rc, msg = call(**kw)
    assert rc == INVALID and NAME[call] in msg and "sizes" in msg
    zero = dict(c=0) if call is _col else dict(n=0)
    assert call(e=2 ** 31 - 1, **zero)[0] == 0       # the largest size itself is in range


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_edges_without_columns_are_refused(call):
    rc, msg = call(c=0)
    assert rc == INVALID and "sizes" in msg


@pytest.mark.parametrize("call", [_fwd, _bwd])
@pytest.mark.parametrize("slope", [math.nan, math.inf, -math.inf])
def test_a_non_finite_slope_is_refused(call, slope):
    rc, msg = call(slope=slope)
    assert rc == INVALID and NAME[call] in msg and "negative_slope" in msg
    assert call(slope=slope, n=0)[0] == INVALID      # before the empty-call return too


OVERLAPS = ([(_fwd, "alpha", w) for w in FWD_PTRS[:-1]] +
            [(_bwd, o, w) for o in ("grad_edge", "grad_er") for w in BWD_PTRS[:6]] +
            [(_bwd, "grad_edge", "grad_er")] +
            [(_col, "out", w) for w in COL_PTRS[:-1]])


@pytest.mark.parametrize("call,out,which", OVERLAPS)
def test_an_output_overlapping_an_input_or_an_output_is_refused(call, out, which):
    size, osize = SIZES[which], SIZES[out]
    zero = dict(c=0) if call is _col else dict(n=0)
    for off, overlaps in [(0, True), (size - 1, True), (1 - osize, True), (size, False),
                          (-osize, False)]:
        kw = {which: P(9 * B), out: P(9 * B + off)}
        rc, msg = call(**kw) if overlaps else call(**kw, **zero)
        if overlaps:
            assert rc == INVALID and "overlaps" in msg, (off, msg)
        else:
            assert rc == 0, (off, msg)   # adjacent ranges with rows run on the GPU
