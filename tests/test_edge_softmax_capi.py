"""CPU: the edge-softmax entry points (maxk_edge_softmax_forward / _backward / _row_limits) are
declared, bound, and refuse bad arguments on the host before any device call; and the float64
restatement and the two error bounds (include/maxk_hip.h, "Edge softmax") that the GPU tests of
test_gpu_edge_softmax.py hold the kernels to, with pinned hand-computed rows."""
import ctypes
import os
import re

import numpy as np
import pytest

from maxk_kernels import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "maxk_hip.h")
P = ctypes.c_void_p
INVALID = -1
U = 2.0 ** -24
TINY = 2.0 ** -126


# ------------------------------------------------------------------ the formulas, in float64
def _rows(ptr):
    ptr = np.asarray(ptr, dtype=np.int64)
    return ptr, np.repeat(np.arange(ptr.size - 1), np.diff(ptr))


def _segment_sum(v, ptr):
    """Sum of v over each row, float64, empty rows 0 (np.add.reduceat mishandles them)."""
    out = np.zeros(ptr.size - 1, dtype=np.float64)
    np.add.at(out, _rows(ptr)[1], v)
    return out


def softmax_rows64(ptr, logits):
    """float64 softmax of the f32 logits over each row [ptr[r], ptr[r + 1]): m = max, d = x - m,
    p = exp(d), out = p / sum p. Non-finite logits follow IEEE through those operations: a NaN
    or +Inf, or a row of only -Inf, makes its row NaN; -Inf beside a finite logit gives 0."""
    ptr, rows = _rows(ptr)
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    m = np.full(ptr.size - 1, -np.inf)
    with np.errstate(all="ignore"):
        np.maximum.at(m, rows, x)                 # propagates NaN
        p = np.exp(x - m[rows])
        return p / _segment_sum(p, ptr)[rows]


def softmax_backward_rows64(ptr, y, grad_y):
    """float64 gradient from the f32 y and grad_y: t = sum y g per row, y (g - t)."""
    ptr, rows = _rows(ptr)
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    g = np.asarray(grad_y, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return y * (g - _segment_sum(y * g, ptr)[rows])


def _blocks(ptr):
    """ceil(n / 64) of each edge's row."""
    ptr, rows = _rows(ptr)
    return (-(-np.diff(ptr) // 64))[rows].astype(np.float64)


def forward_rel_bound(ptr, logits):
    """(2 R + ceil(n / 64) + 20) u per edge, R = max - min of the row's finite logits: the
    subtraction costs R u in the numerator and in the sum, expf 2 ulp = 4 u in both, the sum
    ceil(n / 64) + 6 (>= 64 independent accumulators and a tree), reciprocal and multiply 3."""
    ptr, rows = _rows(ptr)
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    fin = np.isfinite(x)
    hi = np.full(ptr.size - 1, -np.inf)
    lo = np.full(ptr.size - 1, np.inf)
    np.maximum.at(hi, rows[fin], x[fin])
    np.minimum.at(lo, rows[fin], x[fin])
    R = np.where(hi >= lo, hi - lo, 0.0)
    return (2 * R[rows] + _blocks(ptr) + 20) * U


def forward_bound(ptr, logits):
    """|out - y64| <= (2 R + ceil(n / 64) + 20) u y64 + 2^-126."""
    with np.errstate(all="ignore"):
        return forward_rel_bound(ptr, logits) * softmax_rows64(ptr, logits) + TINY


def backward_bound(ptr, y, grad_y):
    """|grad - ref| <= (ceil(n / 64) + 10) u y (|g| + sum |y g|) + 2^-126: the products one
    rounding each, their sum ceil(n / 64) + 6, the difference and the last product one each."""
    ptr, rows = _rows(ptr)
    y = np.abs(np.asarray(y, dtype=np.float32).astype(np.float64))
    g = np.abs(np.asarray(grad_y, dtype=np.float32).astype(np.float64))
    return (_blocks(ptr) + 10) * U * y * (g + _segment_sum(y * g, ptr)[rows]) + TINY


def test_pinned_rows():
    y = softmax_rows64([0, 4], [0, 0, 0, 0])
    assert y.tolist() == [0.25] * 4
    got = softmax_backward_rows64([0, 4], y, [1, 2, 3, 4])
    assert got.tolist() == [-0.375, -0.125, 0.125, 0.375]
    # two rows and an empty one between them; exp(-ln 3) against 1
    y = softmax_rows64([0, 2, 2, 3], np.array([0.0, -np.log(3.0), 7.0], np.float32))
    np.testing.assert_allclose(y, [0.75, 0.25, 1.0], rtol=1e-7)
    assert softmax_backward_rows64([0, 1], [1.0], [5.0]).tolist() == [0.0]


def test_non_finite_rows_follow_ieee():
    inf = np.inf
    ptr = [0, 3, 6, 8, 10, 12]
    x = np.array([0, -inf, 0, 1, np.nan, 2, inf, 0, -inf, -inf, 3, 4], np.float32)
    y = softmax_rows64(ptr, x)
    assert y[:3].tolist() == [0.5, 0.0, 0.5] and not np.signbit(y[1])
    assert np.isnan(y[3:10]).all()                    # NaN row, +Inf row, only -Inf row
    assert np.isfinite(y[10:]).all() and abs(y[10:].sum() - 1) < 1e-15
    g = softmax_backward_rows64(ptr[:2], y[:3], [1.0, 100.0, 3.0])
    assert g.tolist() == [-0.5, 0.0, 0.5]             # the -Inf edge passes no gradient


def test_bounds_on_hand_rows():
    # n = 4, R = 0: (0 + 1 + 20) u
    assert np.all(forward_rel_bound([0, 4], [3, 3, 3, 3]) == 21 * U)
    # n = 65 -> two blocks of 64; R = 1.5 from the finite logits only
    x = np.zeros(65, np.float32)
    x[0], x[1], x[2] = 1.5, -np.inf, 0.25
    assert np.all(forward_rel_bound([0, 65], x) == (3.0 + 2 + 20) * U)
    b = backward_bound([0, 2], [0.5, 0.5], [2.0, -4.0])
    assert b.tolist() == [11 * U * 0.5 * (2 + 3) + TINY, 11 * U * 0.5 * (4 + 3) + TINY]


def _lanes_f32(x, lanes=64):
    """An f32 implementation of the forward with `lanes` strided accumulators and a tree."""
    x = np.asarray(x, np.float32)
    p = np.exp(x - x.max()).astype(np.float32)
    acc = np.zeros(lanes, np.float32)
    for i in range(0, p.size, lanes):
        c = p[i:i + lanes]
        acc[:c.size] = acc[:c.size] + c
    while acc.size > 1:
        acc = acc[0::2] + acc[1::2]
    assert acc.dtype == np.float32
    return p * (np.float32(1) / acc[0])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 5000, 20000])
@pytest.mark.parametrize("R", [0.5, 16.0, 60.0])
def test_an_f32_implementation_stays_inside_the_forward_bound(n, R):
    """The bound is not tuned to the kernel under test: a 64-lane strided f32 numpy
    implementation (numpy's expf) keeps a margin of at least 3 under it."""
    rng = np.random.default_rng(n + int(R))
    x = (rng.random(n) * R).astype(np.float32)
    got = _lanes_f32(x).astype(np.float64)
    err = np.abs(got - softmax_rows64([0, n], x))
    assert np.all(err <= forward_bound([0, n], x) / 3)


@pytest.mark.parametrize("n", [1, 3, 64, 65, 1025, 5000])
def test_an_f32_implementation_stays_inside_the_backward_bound(n):
    rng = np.random.default_rng(n)
    y = _lanes_f32(rng.random(n).astype(np.float32))
    g = rng.standard_normal(n).astype(np.float32)
    prod = y * g
    acc = np.zeros(64, np.float32)
    for i in range(0, n, 64):
        c = prod[i:i + 64]
        acc[:c.size] = acc[:c.size] + c
    while acc.size > 1:
        acc = acc[0::2] + acc[1::2]
    got = (y * (g - acc[0])).astype(np.float64)
    err = np.abs(got - softmax_backward_rows64([0, n], y, g))
    assert np.all(err <= backward_bound([0, n], y, g) / 3)


# ------------------------------------------------------------------ the C entry points
FWD_ARGS = [P, P, P, ctypes.c_int32, ctypes.c_int64, P]
BWD_ARGS = [P, P, P, P, ctypes.c_int32, ctypes.c_int64, P]


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
    assert m, name
    return [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]


def test_header_declares_and_binding_binds_the_entry_points():
    assert _declared("maxk_edge_softmax_forward") == [
        "const int32_t*", "const float*", "float*", "int32_t", "int64_t", "void*"]
    assert _declared("maxk_edge_softmax_backward") == [
        "const int32_t*", "const float*", "const float*", "float*", "int32_t", "int64_t", "void*"]
    assert _declared("maxk_edge_softmax_row_limits") == ["int32_t*", "int32_t"]
    for name, args in [("maxk_edge_softmax_forward", FWD_ARGS),
                       ("maxk_edge_softmax_backward", BWD_ARGS),
                       ("maxk_edge_softmax_row_limits", [P, ctypes.c_int32])]:
        res, sig = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and sig == args
        assert getattr(_lib.lib, name).argtypes == args
    assert _lib.lib.maxk_abi_version() == 4      # new symbols only


def test_row_limits():
    lib = _lib.lib
    count = lib.maxk_edge_softmax_row_limits(None, 0)
    assert count >= 2                            # at least three regimes
    buf = (ctypes.c_int32 * (count + 1))(*([-7] * (count + 1)))
    assert lib.maxk_edge_softmax_row_limits(ctypes.cast(buf, P), count + 1) == count
    limits = list(buf)[:count]
    assert buf[count] == -7 and limits == sorted(set(limits)) and limits[0] >= 1
    assert ops.edge_softmax_row_limits() == tuple(limits)
    short = (ctypes.c_int32 * count)(*([-7] * count))   # capacity below the count
    assert lib.maxk_edge_softmax_row_limits(ctypes.cast(short, P), 1) == count
    assert list(short) == [limits[0]] + [-7] * (count - 1)


B = 1 << 24   # fake device addresses, far apart: nothing is dereferenced on the host


def _fwd(ptr=P(B), logits=P(2 * B), out=P(3 * B), n=10, e=100):
    rc = _lib.lib.maxk_edge_softmax_forward(ptr, logits, out, n, e, None)
    return rc, _lib.lib.maxk_last_error().decode()


def _bwd(ptr=P(B), y=P(2 * B), grad_y=P(3 * B), grad_logits=P(4 * B), n=10, e=100):
    rc = _lib.lib.maxk_edge_softmax_backward(ptr, y, grad_y, grad_logits, n, e, None)
    return rc, _lib.lib.maxk_last_error().decode()


@pytest.mark.parametrize("call,which", [(_fwd, "ptr"), (_fwd, "logits"), (_fwd, "out"),
                                        (_bwd, "ptr"), (_bwd, "y"), (_bwd, "grad_y"),
                                        (_bwd, "grad_logits")])
def test_null_pointers_are_refused(call, which):
    rc, msg = call(**{which: None})
    assert rc == INVALID and "maxk_edge_softmax" in msg and "null pointer" in msg


def test_empty_input_launches_nothing():
    assert _fwd(ptr=None, logits=None, out=None, e=0)[0] == 0
    assert _fwd(ptr=None, logits=None, out=None, n=0, e=0)[0] == 0
    assert _fwd(ptr=None, logits=None, out=None, n=0, e=5)[0] == 0
    none = dict(ptr=None, y=None, grad_y=None, grad_logits=None)
    assert _bwd(e=0, **none)[0] == 0
    assert _bwd(n=0, e=0, **none)[0] == 0
    assert _bwd(n=0, e=5, **none)[0] == 0


@pytest.mark.parametrize("call", [_fwd, _bwd])
@pytest.mark.parametrize("kw", [dict(n=-1), dict(e=-1), dict(e=2 ** 31), dict(e=2 ** 40)])
def test_sizes_out_of_range_are_refused(call, kw):
    rc, msg = call(**kw)
    assert rc == INVALID and "maxk_edge_softmax" in msg and "sizes" in msg
    assert call(e=2 ** 31 - 1, n=0)[0] == 0      # the largest size itself is in range


# the default call's ranges (bytes): ptr 4 * 11, every [E] array 400
@pytest.mark.parametrize("call,out,which,size", [
    (_fwd, "out", "ptr", 44), (_fwd, "out", "logits", 400),
    (_bwd, "grad_logits", "ptr", 44), (_bwd, "grad_logits", "y", 400),
    (_bwd, "grad_logits", "grad_y", 400)])
def test_an_output_overlapping_an_input_is_refused(call, out, which, size):
    for off, overlaps in [(0, True), (size - 1, True), (-399, True), (size, False), (-400, False)]:
        rc, msg = call(**{which: P(5 * B), out: P(5 * B + off), "n": 10 if overlaps else 0})
        if overlaps:
            assert rc == INVALID and "overlaps" in msg, (off, msg)
        else:
            # num_rows = 0: nothing to refuse and still no device call (adjacent ranges with
            # rows run on the GPU: test_gpu_edge_softmax.py::test_adjacent_ranges_are_accepted)
            assert rc == 0, (off, msg)
