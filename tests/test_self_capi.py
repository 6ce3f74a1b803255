"""CPU: the entry points of the self-term path (maxk_topk_cbsr_dense, maxk_scatter_backward_merge)
are declared, bound, and refuse bad arguments on the host before any device call; and the numpy
restatement of their two formulas (include/maxk_hip.h, "Dense masked row and merged gradient"),
which the GPU tests of test_gpu_self.py hold the kernels to bit for bit, with pinned
hand-computed rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from maxk_kernels import _lib
from test_dropout_capi import drop_scale, keep_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
P = ctypes.c_void_p
INVALID = -1


# ------------------------------------------------------------------ the two formulas, in numpy
def dense_rows(values, index, count, D):
    """The dense masked rows of a CBSR table: dense[r, index[r, j]] = values[r, j] (bit pattern)
    for the filled slots j < count[r] (``count=None``: every slot), +0.0f elsewhere."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    index = np.asarray(index)
    n, k = values.shape
    out = np.zeros((n, D), dtype=np.uint32)
    bits = values.view(np.uint32)
    for r in range(n):
        for j in range(k if count is None else int(count[r])):
            out[r, int(index[r, j])] = bits[r, j]
    return out.view(np.float32)


def merge_rows(grad_sp, index, grad_dense, p, seed, row_offset=0, D=None):
    """grad_in of maxk_scatter_backward_merge: for the winning (last) slot j* of feature f,
    s = fl32(grad_dense[r, f] + grad_sp[r, j*]) (the other operand alone when one is None),
    grad_in[r, f] = p == 0 ? s : (keep ? fl32(s * scale) : +0.0f); +0.0f for unselected f."""
    index = np.asarray(index)
    n, k = index.shape
    if D is None:
        D = grad_dense.shape[1]
    winner = np.full((n, D), -1, dtype=np.int64)
    for j in range(k):
        winner[np.arange(n), index[:, j].astype(np.int64)] = j
    sel = winner >= 0
    wj = np.where(sel, winner, 0)
    with np.errstate(all="ignore"):
        if grad_sp is None:
            s = np.asarray(grad_dense, dtype=np.float32).copy()
        else:
            s = np.take_along_axis(np.asarray(grad_sp, dtype=np.float32), wj, axis=1)
            if grad_dense is not None:
                s = (np.asarray(grad_dense, dtype=np.float32) + s).astype(np.float32)
        if np.float32(p) != 0:
            rows = row_offset + np.arange(n, dtype=np.int64)[:, None]
            keep = keep_mask(p, seed, rows, np.arange(D)[None, :])
            s = np.where(keep, (s * drop_scale(p)).astype(np.float32), np.float32(0.0))
    out = np.zeros((n, D), dtype=np.uint32)
    out[sel] = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)[sel]
    return out.view(np.float32)


def test_dense_rows_pinned():
    v = np.array([[1.5, -0.0, 3.0], [7.0, 0.0, 0.0]], dtype=np.float32)
    i = np.array([[1, 4, 6], [5, 0, 0]], dtype=np.uint8)
    got = dense_rows(v, i, None, 8)
    assert got[0].tolist() == [0, 1.5, 0, 0, 0, 0, 3.0, 0]
    assert got.view(np.uint32)[0, 4] == 0x80000000          # a selected -0.0f keeps its sign
    # ref_compat row with one filled slot: the padding slots (0.0f, 0) write nothing
    got = dense_rows(v, i, np.array([3, 1]), 8)
    assert got[1].tolist() == [0, 0, 0, 0, 0, 7.0, 0, 0]
    assert not got.view(np.uint32)[1, [0, 1, 2, 3, 4, 6, 7]].any()


def test_merge_rows_pinned():
    gs = np.array([[1.0, 2.0, 4.0, 8.0]], dtype=np.float32)
    ix = np.array([[2, 5, 2, 7]], dtype=np.uint8)             # feature 2 twice: slot 2 wins
    gd = np.array([[np.nan, 10, 0.5, np.inf, 10, 0.25, 10, -8.0]], dtype=np.float32)
    got = merge_rows(gs, ix, gd, 0.0, 0)
    assert got[0].tolist() == [0, 0, 4.5, 0, 0, 2.25, 0, 0]  # NaN / Inf at unselected features
    assert not got.view(np.uint32)[0, [0, 1, 3, 4, 6, 7]].any()   # ... are +0.0f exactly
    assert merge_rows(None, ix, gd, 0.0, 0)[0].tolist() == [0, 0, 0.5, 0, 0, 0.25, 0, -8.0]
    assert merge_rows(gs, ix, None, 0.0, 0, D=8)[0].tolist() == [0, 0, 4.0, 0, 0, 2.0, 0, 8.0]
    # p = 0.5: scale 2 on the kept sums, +0.0f on the dropped ones
    keep = keep_mask(0.5, 9, np.array([[3]]), np.arange(8)[None, :])[0]
    got = merge_rows(gs, ix, gd, 0.5, 9, row_offset=3)
    want = [0, 0, 9.0 * keep[2], 0, 0, 4.5 * keep[5], 0, 0]
    assert got[0].tolist() == want
    assert not merge_rows(gs, ix, gd, 1.0, 9).view(np.uint32).any()


# ------------------------------------------------------------------ the C entry points
def test_header_declares_and_binding_binds_the_self_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("maxk_topk_cbsr_dense", "maxk_scatter_backward_merge"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib, name)
    assert _lib.lib.maxk_abi_version() == 4      # new symbols only


def _topk(inp=None, dense=P(1 << 20), dense_stride=0, k=16, d=256, n=10, p=0.5, row_offset=0,
          records=None, record_bytes=0, layout=0, mode=0):
    rc = _lib.lib.maxk_topk_cbsr_dense(inp, dense, dense_stride, records, record_bytes, layout,
                                       None, 0, None, 0, None, None, None, 0, n, d, k, mode, p,
                                       12345, row_offset, None)
    return rc, _lib.lib.maxk_last_error().decode()


def _merge(grad_sp=None, grad_dense=P(1 << 20), dense_stride=0, grad_in=None, p=0.5,
           row_offset=0, n=10, d=256, k=16):
    rc = _lib.lib.maxk_scatter_backward_merge(grad_sp, None, 0, grad_dense, dense_stride,
                                              grad_in, n, d, k, p, 12345, row_offset, None)
    return rc, _lib.lib.maxk_last_error().decode()


def test_null_dense_is_refused():
    for p in (0.0, 0.5):
        rc, msg = _topk(dense=None, p=p)
        assert rc == INVALID and "maxk_topk_cbsr_dense" in msg and "dense is null" in msg
        rc, msg = _topk(dense=None, p=p, n=0)
        assert rc == INVALID and "dense is null" in msg


@pytest.mark.parametrize("stride", [1, 255, -4])
def test_dense_stride_below_the_row_is_refused(stride):
    rc, msg = _topk(dense_stride=stride)
    assert rc == INVALID and "maxk_topk_cbsr_dense" in msg and "dense_stride" in msg
    rc, msg = _merge(grad_sp=P(4096), dense_stride=stride)
    assert rc == INVALID and "maxk_scatter_backward_merge" in msg and "dense_stride" in msg
    assert _topk(dense_stride=100, d=100, n=0)[0] == 0       # the row itself is allowed


def test_both_gradients_null_is_refused():
    for p in (0.0, 0.5):
        rc, msg = _merge(grad_sp=None, grad_dense=None, p=p)
        assert rc == INVALID and "maxk_scatter_backward_merge" in msg and "both null" in msg


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan"), float("inf")])
def test_probability_out_of_range_is_refused(p):
    rc, msg = _topk(p=p)
    assert rc == INVALID and "maxk_topk_cbsr_dense" in msg and "p must" in msg
    rc, msg = _merge(p=p)
    assert rc == INVALID and "maxk_scatter_backward_merge" in msg and "p must" in msg


def test_negative_row_offset_is_refused():
    for p in (0.0, 0.5):
        rc, msg = _topk(p=p, row_offset=-1)
        assert rc == INVALID and "maxk_topk_cbsr_dense" in msg and "row_offset" in msg
        rc, msg = _merge(p=p, row_offset=-1)
        assert rc == INVALID and "maxk_scatter_backward_merge" in msg and "row_offset" in msg


@pytest.mark.parametrize("off,stride,overlaps", [
    (0, 0, True),                    # the same buffer
    (4 * (10 * 256 - 1), 0, True),   # dense starts at the last float of in
    (-4 * (10 * 256 - 1), 0, True),  # dense ends at the first float of in
    (-4 * (9 * 300 + 255), 300, True),   # strided: the last row's last float
    (4 * 10 * 256, 0, False),        # right behind in
    (-4 * 10 * 256, 0, False),       # right in front of it
    (-4 * (9 * 300 + 256), 300, False),
])
def test_dense_overlapping_in_is_refused(off, stride, overlaps):
    base = 1 << 24
    for p in (0.0, 0.5):
        # an unknown mode is what refuses the ranges that do not overlap: no device call
        rc, msg = _topk(inp=P(base), dense=P(base + off), dense_stride=stride, p=p, mode=9)
        assert rc == INVALID
        assert ("overlaps" in msg) == overlaps and ("unknown mode" in msg) != overlaps, msg
    # grad_in against grad_dense
    rc, msg = _merge(grad_sp=P(4096), grad_in=P(base), grad_dense=P(base + off),
                     dense_stride=stride)
    assert rc == INVALID and ("overlaps" in msg) == overlaps, msg


def test_tables_and_records_are_all_optional():
    """Without records and tables only the null input is left to refuse (N > 0); N = 0 is a
    no-op. Record arguments, when given, follow maxk_topk_cbsr_records."""
    rc, msg = _topk()
    assert rc == INVALID and "null pointer" in msg
    assert _topk(n=0)[0] == 0 and _topk(n=0, p=0.0)[0] == 0
    rc, msg = _topk(records=P(4096 + 8), record_bytes=128, layout=4)
    assert rc == INVALID and "16-B aligned" in msg
    rc, msg = _topk(records=P(4096), record_bytes=128, layout=3)
    assert rc == -2 and "maxk_topk_cbsr_dense" in msg
    rc, msg = _topk(k=300)
    assert rc == INVALID
    rc, msg = _topk(d=257)
    assert rc == INVALID and "dim_origin" in msg


def test_merge_null_pointers_and_empty_input():
    rc, msg = _merge(grad_sp=P(4096))               # selectors and grad_in are null
    assert rc == INVALID and "null pointer" in msg
    assert _merge(n=0)[0] == 0 and _merge(n=0, p=0.0)[0] == 0


def test_fake_kernels_of_the_self_operators():
    with FakeTensorMode():
        x = torch.empty(50, 64, device="cuda")
        dense, sp_data, sp_index = torch.ops.maxk.maxk_dense_forward(x, 16, 0.5, -3)
        assert dense.shape == (50, 64) and dense.dtype == torch.float32
        assert sp_data.shape == (50, 16) and sp_data.dtype == torch.float32
        assert sp_index.shape == (50, 16) and sp_index.dtype == torch.uint8
        g = torch.ops.maxk.maxk_merge_backward(sp_data, sp_index, dense, 0.5, -3)
        assert g.shape == (50, 64) and g.device.type == "cuda"
