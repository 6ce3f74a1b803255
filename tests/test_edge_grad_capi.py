"""CPU: the edge-value gradient entry point (maxk_sddmm_edge_grad) is declared, bound, and
refuses bad arguments on the host before any device call; and the numpy restatement of its
summation tree (include/maxk_hip.h, "Edge-value gradient"), which the GPU tests of
test_gpu_edge_grad.py hold the kernel to bit for bit, with pinned hand-computed rows."""
import ctypes
import os
import re

import numpy as np
import pytest

from maxk_kernels import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
P = ctypes.c_void_p
INVALID, UNSUPPORTED = -1, -2
U = 2.0 ** -24


# ------------------------------------------------------------------ the formula, in numpy
def edge_grad_rows(ptr, idx, G, values, index):
    """grad_val of maxk_sddmm_edge_grad: for edge e = (r, c), t_l = fl32(values[c, l] *
    G[r, index[c, l]]) for l < k and +0.0f up to K2 (the next power of two >= k), then
    t_l = fl32(t_l + t_{l ^ s}) for s = 1, 2, 4, ..., K2 / 2, all l at once; grad_val[e] = t_0.
    Only np.float32 multiplies and adds (no np.sum)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    G = np.asarray(G, dtype=np.float32)
    values = np.asarray(values, dtype=np.float32)
    index = np.asarray(index).astype(np.int64)
    k = values.shape[1]
    K2 = 1
    while K2 < k:
        K2 *= 2
    rows = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    t = np.zeros((idx.size, K2), dtype=np.float32)
    with np.errstate(all="ignore"):
        t[:, :k] = values[idx] * G[rows[:, None], index[idx]]
        assert t.dtype == np.float32
        lanes = np.arange(K2)
        s = 1
        while s < K2:
            t = t + t[:, lanes ^ s]
            assert t.dtype == np.float32
            s *= 2
    return np.ascontiguousarray(t[:, 0])


def gamma(k):
    return k * U / (1 - k * U)


def _one_edge(x, g=None):
    """The tree sum of the products x[l] * g[l] (g: ones) through edge_grad_rows: one edge
    (0, 0) whose row selects features 0 .. k-1."""
    x = np.asarray(x, dtype=np.float32)[None, :]
    k = x.shape[1]
    g = np.ones((1, k), np.float32) if g is None else np.asarray(g, dtype=np.float32)[None, :]
    return edge_grad_rows([0, 1], [0], g, x, np.arange(k)[None, :])[0]


def test_pinned_rows():
    assert _one_edge([1, 2, 3], [0.5, 0.25, 2]) == 7.0            # (0.5 + 0.5) + (6 + 0)
    assert _one_edge([1, 2, 3, 4, 5], [1, 1, 1, 1, 2]) == 20.0    # K2 = 8
    # selectors pick the features, repeated ones included
    G = np.array([[10, 20, 30, 40], [1, 2, 3, 4]], dtype=np.float32)
    v = np.array([[1, 1, 1], [2, 0.5, -1]], dtype=np.float32)
    ix = np.array([[3, 3, 0], [1, 2, 2]], dtype=np.uint8)
    got = edge_grad_rows([0, 2, 3], [0, 1, 1], G, v, ix)
    assert got.tolist() == [90.0, 25.0, 2.5]


def test_signed_zeros_follow_the_tree():
    # k = 1: no add at all, the product's own sign survives
    assert np.float32(_one_edge([-1.0], [0.0])).view(np.uint32) == 0x80000000
    # k = 2: (-0) + (-0) = -0
    assert np.float32(_one_edge([-1.0, -2.0], [0.0, 0.0])).view(np.uint32) == 0x80000000
    # k = 3: the padding slot is +0.0f, so ((-0) + (-0)) + ((-0) + (+0)) = +0
    assert np.float32(_one_edge([-1.0, -2.0, -3.0], [0.0, 0.0, 0.0])).view(np.uint32) == 0


def test_the_order_is_what_is_pinned():
    """(1e8 + 1) + (-1e8 + 1) = 1e8 + -1e8 = 0 in the tree; left to right it is
    ((1e8 + 1) + -1e8) + 1 = 0 + 1 = 1."""
    x = np.array([1e8, 1, -1e8, 1], dtype=np.float32)
    left = np.float32(0)
    for v in x:
        left = np.float32(left + v)
    assert left == 1.0
    assert _one_edge(x) == 0.0


def test_non_finite_values_follow_ieee():
    inf = np.inf
    assert np.isnan(_one_edge([inf, 1.0], [0.0, 1.0]))            # Inf * 0
    assert np.isnan(_one_edge([inf, -inf, 1, 1]))
    assert _one_edge([inf, 1, 1]) == inf
    assert _one_edge([1.0], [-inf]) == -inf
    # a padding slot never multiplies: k = 3 of all-Inf gradients has no 0 * Inf
    assert _one_edge([1, 1, 1], [inf, inf, inf]) == inf


@pytest.mark.parametrize("k,d", [(1, 8), (2, 8), (3, 8), (7, 16), (16, 64), (24, 64), (64, 256)])
def test_restatement_against_float64(k, d):
    """|tree - exact| <= gamma_k * sum |x g|: each product carries one rounding and passes
    through log2(K2) adds, 1 + log2(K2) <= k roundings on every path, so the standard bound
    (1 + u)^k - 1 <= gamma_k = k u / (1 - k u), u = 2^-24, covers it. Inputs are finite and far
    from underflow, so no term loses more than its relative rounding."""
    rng = np.random.default_rng(k * 1000 + d)
    n, nc, e = 40, 30, 500
    deg = rng.multinomial(e, np.ones(n) / n)
    ptr = np.concatenate([[0], np.cumsum(deg)])
    idx = rng.integers(0, nc, e)
    G = rng.standard_normal((n, d)).astype(np.float32)
    v = rng.standard_normal((nc, k)).astype(np.float32)
    ix = rng.integers(0, d, (nc, k)).astype(np.uint8)
    got = edge_grad_rows(ptr, idx, G, v, ix)
    rows = np.repeat(np.arange(n), deg)
    prod = v[idx].astype(np.float64) * G[rows[:, None], ix[idx].astype(np.int64)].astype(np.float64)
    exact, mag = prod.sum(1), np.abs(prod).sum(1)
    assert np.all(np.abs(got.astype(np.float64) - exact) <= gamma(k) * mag)


# ------------------------------------------------------------------ the C entry point
ARGTYPES = [P, P, P, ctypes.c_int64, P, ctypes.c_int64, P, ctypes.c_int64, P, ctypes.c_int32,
            ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, P]


def test_header_declares_and_binding_binds_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+maxk_sddmm_edge_grad\s*\(([^)]*)\)", text)
    assert m
    types = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]
    assert types == ["const int32_t*", "const int32_t*", "const float*", "int64_t", "const float*",
                     "int64_t", "const uint8_t*", "int64_t", "float*", "int32_t", "int32_t",
                     "int64_t", "int32_t", "int32_t", "void*"]
    res, args = _lib.SIGNATURES["maxk_sddmm_edge_grad"]
    assert res is ctypes.c_int and args == ARGTYPES
    assert _lib.lib.maxk_sddmm_edge_grad.argtypes == ARGTYPES
    assert _lib.lib.maxk_abi_version() == 4      # a new symbol only


B = 1 << 24   # fake device addresses, far apart: nothing is dereferenced on the host


def _call(ptr=P(B), idx=P(2 * B), grad_out=P(3 * B), gs=0, sp_data=P(4 * B), ds=0,
          sp_index=P(5 * B), is_=0, grad_val=P(6 * B), n=10, nc=10, e=100, d=64, k=16):
    rc = _lib.lib.maxk_sddmm_edge_grad(ptr, idx, grad_out, gs, sp_data, ds, sp_index, is_,
                                       grad_val, n, nc, e, d, k, None)
    return rc, _lib.lib.maxk_last_error().decode()


@pytest.mark.parametrize("which", ["ptr", "idx", "grad_out", "sp_data", "sp_index", "grad_val"])
def test_null_pointers_are_refused(which):
    rc, msg = _call(**{which: None})
    assert rc == INVALID and "maxk_sddmm_edge_grad" in msg and "null pointer" in msg


def test_empty_input_launches_nothing():
    none = dict(ptr=None, idx=None, grad_out=None, sp_data=None, sp_index=None, grad_val=None)
    assert _call(e=0, **none)[0] == 0
    assert _call(n=0, e=0, **none)[0] == 0
    assert _call(n=0, e=5, **none)[0] == 0


@pytest.mark.parametrize("kw", [dict(n=-1), dict(nc=-1), dict(e=-1)])
def test_negative_sizes_are_refused(kw):
    rc, msg = _call(**kw)
    assert rc == INVALID and "maxk_sddmm_edge_grad" in msg and "sizes" in msg


@pytest.mark.parametrize("d,k", [(64, 0), (64, -3), (64, 65), (260, 16), (0, 0), (512, 512)])
def test_k_and_dim_out_of_range_are_refused(d, k):
    rc, msg = _call(d=d, k=k)
    assert rc == INVALID and "maxk_sddmm_edge_grad" in msg


@pytest.mark.parametrize("d", [6, 63, 255])
def test_dim_not_a_multiple_of_4_is_unsupported(d):
    rc, msg = _call(d=d, k=2)
    assert rc == UNSUPPORTED and "multiple of 4" in msg


@pytest.mark.parametrize("kw,word", [(dict(gs=63), "grad_stride"), (dict(gs=-64), "grad_stride"),
                                     (dict(ds=15), "data_stride"), (dict(ds=-1), "data_stride"),
                                     (dict(is_=15), "index_stride"), (dict(is_=-16), "index_stride")])
def test_strides_below_the_row_are_refused(kw, word):
    rc, msg = _call(**kw)
    assert rc == INVALID and word in msg


# input ranges of the default call (bytes): ptr 4 * 11, idx 4 * 100, grad_out 4 * 10 * 64;
# strided: grad_out 4 * (9 * 68 + 64), sp_data 4 * (9 * 20 + 16), sp_index 9 * 80 + 16
@pytest.mark.parametrize("which,size,kw", [
    ("ptr", 44, {}), ("idx", 400, {}), ("grad_out", 2560, {}),
    ("grad_out", 4 * (9 * 68 + 64), dict(gs=68)),
])
def test_grad_val_overlapping_an_input_is_refused(which, size, kw):
    """grad_val is 400 B. With num_cols = 0 a call whose ranges do not overlap is refused by the
    check behind the overlap check (so still no device call), which tells the two apart."""
    for off, overlaps in [(0, True), (size - 1, True), (-399, True), (size, False), (-400, False)]:
        rc, msg = _call(**{which: P(B)}, grad_val=P(B + off), nc=0, **kw)
        assert rc == INVALID
        assert ("overlaps" in msg) == overlaps and ("num_cols" in msg) != overlaps, (off, msg)


@pytest.mark.parametrize("which,size,kw", [
    ("sp_data", 640, {}), ("sp_index", 160, {}),
    ("sp_data", 4 * (9 * 20 + 16), dict(ds=20)), ("sp_index", 9 * 80 + 16, dict(is_=80)),
])
def test_grad_val_overlapping_a_table_is_refused(which, size, kw):
    for off in (0, size - 1, -399):
        rc, msg = _call(**{which: P(B)}, grad_val=P(B + off), **kw)
        assert rc == INVALID and "overlaps" in msg, (off, msg)
