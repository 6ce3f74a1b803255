"""GPU: maxk_max_aggregate_forward / _backward, their autograd Function and operators, and
MaxKSAGEConv's pool and gcn aggregators, against the restatements of tests/max_aggregate.py.
max does not round, so the forward (out, arg_edge, arg_slot) is compared bit for bit on every
input; the backward bit for bit on exactly summable gradients and within the derived bound of
include/maxk_hip.h ("Max aggregation") on real ones. One 600-row graph serves the module: its
row and column lengths sit on both sides of every limit the library reports and include a hub
row of 5,000 and a hub column of 3,000 edges. The last test closes over the compiled maxk_mx::
instantiations: each was launched by a passing case that asserted its restated name.

Worst error / bound figures print with -s."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import max_aggregate as mx
import maxk_kernels as mk
from arena import POISONS, arena
from maxk_kernels import _lib, ops, pooling

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_instantiations_max.txt")
COVERED = set()      # kernel names launched by a case that went on to pass
P = ctypes.c_void_p
NUM = mx.NUM


def dev_of(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype)
    if got.dtype == np.float32:
        got, want = mx.bits(got), mx.bits(want)
    diff = got != want
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def same_forward(got, want, what):
    for g, w, name in zip(got, want, ("out", "arg_edge", "arg_slot")):
        same_bits(g.cpu().numpy(), w, f"{what}: {name}")


@functools.lru_cache(maxsize=None)
def structure():
    ptr, idx = mx.graph_arrays()
    return ptr, idx, mx.transposed(ptr, idx, NUM)


def graph_dev(dev):
    ptr, idx, (pt, it, order) = structure()
    return tuple(dev_of(a, dev) for a in (ptr, idx, pt, it, order))


def launch_names(k, arg=(False, True)):
    """The instantiations a call with k slots launches, by the restated selectors; checked
    against the fixture before anything runs."""
    names = tuple(mx.fwd_kernel_name(k, a) for a in arg) + (mx.bwd_kernel_name(k),)
    with open(FIXTURE) as f:
        compiled = {ln.strip() for ln in f if ln.strip()}
    assert set(names) <= compiled, names
    return names


def fwd(dev, data, sel, D, with_arg=True, graph=None):
    ptr, idx = (graph or graph_dev(dev))[:2]
    return ops.max_aggregate_forward(ptr, idx, data, sel, D, with_arg)


def bwd(dev, g, ae, sl, sel, graph=None):
    pt, it, order = (graph or graph_dev(dev))[2:]
    return ops.max_aggregate_backward(pt, it, order, g, ae, sl, sel)


def test_limits_are_the_restated_ones(gpu):
    assert ops.max_row_limits() == mx.LIMITS


# ------------------------------------------------------------------ 1. forward, bit for bit
@functools.lru_cache(maxsize=None)
def normal_case(D, k):
    ptr, idx, _ = structure()
    data, sel = mx.case_tables(D, k, exact=False, seed=1)
    return (data, sel) + mx.forward_ref(ptr, idx, data, sel, D)


def strided(t, stride):
    buf = torch.zeros((t.shape[0], stride), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def records(data, sel):
    """Layout-1 records (k values, then k selectors, per column) and the two views into them."""
    k = data.shape[1]
    rb = 64 if 5 * k <= 64 else 128 if 5 * k <= 128 else (5 * k + 15) // 16 * 16
    rec = torch.zeros((data.shape[0], rb), dtype=torch.uint8, device=data.device)
    rec[:, :4 * k] = data.contiguous().view(torch.uint8)
    rec[:, 4 * k:5 * k] = sel
    return rec[:, :4 * k].view(torch.float32), rec[:, 4 * k:5 * k]


# layout-1 records exist for k % 4 == 0 only
FORWARD_CASES = [(D, k, layout) for D, k in mx.SHAPES
                 for layout in ("plain", "strided", "records") if layout != "records" or k % 4 == 0]


@pytest.mark.parametrize("D,k,layout", FORWARD_CASES)
def test_forward_matches_the_restatement_bit_for_bit(gpu, D, k, layout):
    names = launch_names(k)[:2]
    for kind, case in (("exact", mx.exact_case), ("normal", normal_case)):
        data, sel, out, ae, sl = case(D, k)
        data, sel = dev_of(data, gpu), dev_of(sel, gpu)
        if layout == "strided":
            data, sel = strided(data, k + 3), strided(sel, k + 5)
        elif layout == "records":
            data, sel = records(data, sel)
        same_forward(fwd(gpu, data, sel, D), (out, ae, sl), f"{kind} tables")
        alone, none_e, none_s = fwd(gpu, data, sel, D, with_arg=False)
        assert none_e is None and none_s is None
        same_bits(alone.cpu().numpy(), out, f"{kind} tables: out without arg_*")
    COVERED.update(names)


# ------------------------------------------------------------------ 2. special values
def test_special_values_follow_the_order(gpu):
    """Hand-made candidates for feature 3 of a 10-row graph: signed zeros, infinities and NaNs
    against each other and against the implicit zero, each expectation written out."""
    D, k, S = 64, 8, 3
    nan_a, nan_b = (np.array([b], np.uint32).view(np.float32)[0] for b in (0x7fc00123, 0xffc00456))
    rng = np.random.default_rng(7)
    sel = np.tile(np.arange(10, 10 + k, dtype=np.uint8), (10, 1))       # none selects feature 3
    data = rng.standard_normal((10, k)).astype(np.float32)
    plant = {0: -0.0, 1: 0.0, 2: np.inf, 3: nan_a, 4: nan_b, 5: -0.0, 6: -np.inf, 8: 0.0}
    for c, v in plant.items():
        sel[c, 0], data[c, 0] = S, v                                   # column 7 and 9: no slot
    rows = [[0, 1], [2, 3], [3, 4], [4, 3], [5], [5, 7], [6, 7], [6], [8, 7], [2, 6, 0]]
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    idx = np.concatenate(rows).astype(np.int32)
    want = [(0x00000000, 1), (0x7fc00123, 1), (0x7fc00123, 0), (0xffc00456, 0), (0x80000000, 0),
            (0x00000000, -1), (0x00000000, -1), (0xff800000, 0), (0x00000000, 0),
            (0x7f800000, 0)]
    ref = mx.forward_ref(ptr, idx, data, sel, D)
    for r, (b, j) in enumerate(want):
        assert mx.bits(ref[0])[r, S] == b and ref[1][r, S] == (ptr[r] + j if j >= 0 else -1), r
    got = ops.max_aggregate_forward(dev_of(ptr, gpu), dev_of(idx, gpu), dev_of(data, gpu),
                                    dev_of(sel, gpu), D)
    same_forward(got, ref, "hand-made special values")


def test_special_values_stay_in_their_rows(gpu):
    D, k = 256, 16
    ptr, idx, _ = structure()
    data, sel, out0, ae0, sl0 = normal_case(D, k)
    data = data.copy()
    cols = {20: np.nan, 21: np.inf, 22: -np.inf, 23: -0.0, 24: 0.0, 300: np.nan, 301: np.inf}
    for c, v in cols.items():
        data[c, c % k] = v
    ref = mx.forward_ref(ptr, idx, data, sel, D)
    got = fwd(gpu, dev_of(data, gpu), dev_of(sel, gpu), D)
    same_forward(got, ref, "planted special values")
    touched = np.unique(mx.rows_of(ptr)[np.isin(idx, list(cols))])
    keep = ~np.isin(np.arange(NUM), touched)
    assert 0 < touched.size and keep.sum() > 50
    out = got[0].cpu().numpy()
    same_bits(out[keep], out0[keep], "rows without an edge to a planted column")
    assert np.isnan(out[touched]).any() and np.isposinf(out[touched]).any()
    assert np.isfinite(out[keep]).all()


# ------------------------------------------------------------------ 3. repeated selectors
@pytest.mark.parametrize("make,D,k", [(mx.padded_tables, 64, 8), (mx.repeated_tables, 256, 16),
                                      (mx.repeated_tables, 256, 100)])
def test_repeated_selectors_are_candidates_of_their_own(gpu, make, D, k):
    ptr, idx, _ = structure()
    data, sel = make(D, k, seed=5)
    ref = mx.forward_ref(ptr, idx, data, sel, D)
    assert mx.classes(ptr, idx, data, sel, D, *ref)["slot_tie"]
    data_d, sel_d = dev_of(data, gpu), dev_of(sel, gpu)
    got = fwd(gpu, data_d, sel_d, D)
    same_forward(got, ref, make.__name__)
    g = mx.exact_grad(NUM, D, seed=k)
    gsp, mag, _ = mx.backward64(ptr, idx, g, ref[1], ref[2], sel)
    assert mag.max() * 2 < 2 ** 24
    same_bits(bwd(gpu, dev_of(g, gpu), got[1], got[2], sel_d).cpu().numpy(),
              gsp.astype(np.float32), make.__name__ + ": grad_sp")


# ------------------------------------------------------------------ 4. position independence
def test_rows_keep_their_bits_elsewhere(gpu):
    D, k = 256, 16
    ptr, idx, _ = structure()
    data, sel, out, ae, sl = mx.exact_case(D, k)
    data_d, sel_d = dev_of(data, gpu), dev_of(sel, gpu)
    rlen = np.diff(ptr)
    picks = [int(np.argmax(rlen))] + [int(np.flatnonzero(rlen == n)[0])
                                      for n in (100, 2, mx.LIMITS[0] + 1, mx.LIMITS[0], 1)]
    segs = [idx[ptr[r]:ptr[r + 1]] for r in picks]
    ptr2, idx2, where = mx.moved_graph(segs, (1, 2, 3, 0, 2, 1), seed=5)
    assert ptr2.size != ptr.size and [int(ptr2[w]) % 4 for w in where] == [1, 2, 3, 0, 2, 1]
    out2, ae2, sl2 = (t.cpu().numpy() for t in ops.max_aggregate_forward(
        dev_of(ptr2, gpu), dev_of(idx2, gpu), data_d, sel_d, D))
    for r, w in zip(picks, where):
        what = f"row {r} of {rlen[r]} edges moved to {w}"
        same_bits(out2[w], out[r], what)
        same_bits(sl2[w], sl[r], what + ": arg_slot")
        same_bits(np.where(ae2[w] >= 0, ae2[w] - ptr2[w], -1),
                  np.where(ae[r] >= 0, ae[r] - ptr[r], -1), what + ": arg_edge - segment start")
    # the whole second graph against the restatement, and a repeated call
    ref2 = mx.forward_ref(ptr2, idx2, data, sel, D)
    for a, b, name in zip((out2, ae2, sl2), ref2, ("out", "arg_edge", "arg_slot")):
        same_bits(a, b, "second graph: " + name)
    same_forward(fwd(gpu, data_d, sel_d, D), (out, ae, sl), "repeated call")


# ------------------------------------------------------------------ 5. backward
@functools.lru_cache(maxsize=None)
def exact_backward(D, k):
    ptr, idx, _ = structure()
    _, sel, _, ae, sl = mx.exact_case(D, k)
    g = mx.exact_grad(NUM, D, seed=D + k)
    gsp, mag, _ = mx.backward64(ptr, idx, g, ae, sl, sel)
    assert mag.max() * 2 < 2 ** 24          # exactly summable: quanta of 1/2
    return g, gsp.astype(np.float32)


@pytest.mark.parametrize("D,k", mx.SHAPES)
def test_backward_matches_the_restatement_bit_for_bit(gpu, D, k):
    names = launch_names(k)[2:]
    _, sel, _, ae, sl = mx.exact_case(D, k)
    g, gsp = exact_backward(D, k)
    sel_d, ae_d, sl_d, g_d = (dev_of(a, gpu) for a in (sel, ae, sl, g))
    same_bits(bwd(gpu, g_d, ae_d, sl_d, sel_d).cpu().numpy(), gsp, "grad_sp")
    same_bits(bwd(gpu, strided(g_d, D + 4), ae_d, sl_d, strided(sel_d, k + 5)).cpu().numpy(), gsp,
              "grad_sp, strided grad_out and sp_index")
    COVERED.update(names)


@pytest.mark.parametrize("D,k", mx.SHAPES)
def test_backward_is_within_the_derived_bound(gpu, D, k):
    ptr, idx, (pt, _, _) = structure()
    _, sel, _, ae, sl = normal_case(D, k)
    g = np.random.default_rng(k).standard_normal((NUM, D)).astype(np.float32)
    got = bwd(gpu, *(dev_of(a, gpu) for a in (g, ae, sl, sel)))
    again = bwd(gpu, *(dev_of(a, gpu) for a in (g, ae, sl, sel)))
    same_bits(again.cpu().numpy(), got.cpu().numpy(), "two calls")
    ref, mag, m = mx.backward64(ptr, idx, g, ae, sl, sel)
    err, bnd = np.abs(got.cpu().numpy() - ref), mx.bound(mag, m)
    with np.errstate(all="ignore"):
        ratio = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    reg = np.digitize(np.repeat(np.diff(pt), k).reshape(-1, k), mx.LIMITS[2:], right=True)
    w = [float(ratio[reg == r].max(initial=0.0)) for r in range(3)]
    print(f"\ngrad_sp (D, k) = ({D}, {k}): worst error / bound per regime "
          f"{['%.3f' % v for v in w]}, most terms {int(m.max())}")
    assert np.isfinite(ratio).all() and max(w) <= 1.0, w
    assert m.max() <= np.diff(pt).max()


@pytest.mark.parametrize("D,k", mx.TABLE_SHAPES[:4])
def test_every_gradient_element_is_received_exactly_once(gpu, D, k):
    """With the winners of the dense restatement: what arrives in grad_sp is, exactly, what
    grad_out holds where an explicit candidate won."""
    ptr, idx, _ = structure()
    data, sel, out, ae, sl = mx.exact_case(D, k)
    dense = mx.dense_ref(ptr, idx, data, sel, D)
    for a, b, name in zip(dense, (out, ae, sl), ("out", "arg_edge", "arg_slot")):
        same_bits(a, b, "dense restatement: " + name)
    g, _ = exact_backward(D, k)
    got = bwd(gpu, *(dev_of(a, gpu) for a in (g, dense[1], dense[2], sel))).cpu().numpy()
    assert got.astype(np.float64).sum() == g[dense[1] >= 0].astype(np.float64).sum()
    # and per column: the elements whose winner is an edge of that column
    won = dense[1] >= 0
    per_col = np.zeros(NUM)
    np.add.at(per_col, idx[dense[1][won]], g[won].astype(np.float64))
    assert np.array_equal(got.astype(np.float64).sum(axis=1), per_col)


# ------------------------------------------------------------------ 6. output contract
def call_fwd(ptr, idx, data, sel, out_ptr, ae_ptr, sl_ptr, n, nc, e, D, k):
    return _lib.lib.maxk_max_aggregate_forward(
        ops._p(ptr), ops._p(idx), ops._p(data), 0, ops._p(sel), 0, P(out_ptr), P(ae_ptr),
        P(sl_ptr), n, nc, e, D, k, ops._stream())


def call_bwd(pt, it, order, g, ae, sl, sel, sp_ptr, n, nc, e, D, k):
    return _lib.lib.maxk_max_aggregate_backward(
        ops._p(pt), ops._p(it), ops._p(order), ops._p(g), 0, ops._p(ae), ops._p(sl), ops._p(sel),
        0, P(sp_ptr), n, nc, e, D, k, ops._stream())


@pytest.mark.parametrize("poison", POISONS)
def test_output_contract(gpu, poison):
    D, k = 256, 16
    names = launch_names(k)
    ptr, idx, pt, it, order = graph_dev(gpu)
    data, sel, out, ae, sl = mx.exact_case(D, k)
    g, gsp = exact_backward(D, k)
    ins = [dev_of(a, gpu) for a in (data, sel, g, ae, sl)]
    keep = [t.clone() for t in ins + [ptr, idx, pt, it, order]]
    data_d, sel_d, g_d, ae_d, sl_d = ins
    n, e = NUM, idx.numel()
    arenas = [arena((n, D, dt), gpu, poison) for dt in (torch.float32, torch.int32, torch.uint8)]
    assert call_fwd(ptr, idx, data_d, sel_d, *(a.ptr for a in arenas), n, n, e, D, k) == 0
    torch.cuda.synchronize()
    for a, want, name in zip(arenas, (out, ae, sl), ("out", "arg_edge", "arg_slot")):
        assert a.check() is None, name
        same_bits(a.payload.cpu().numpy(), want, name + " in the arena")
    assert arenas[0].first_poisoned() is None and arenas[2].first_poisoned() is None
    empty = np.diff(mx.graph_arrays()[0]) == 0
    assert empty.sum() >= 2 and not mx.bits(arenas[0].payload.cpu().numpy()[empty]).any()
    assert (arenas[1].payload.cpu().numpy()[empty] == -1).all()
    # out alone: arg_* untouched
    a_out = arena((n, D, torch.float32), gpu, poison)
    assert call_fwd(ptr, idx, data_d, sel_d, a_out.ptr, 0, 0, n, n, e, D, k) == 0
    torch.cuda.synchronize()
    assert a_out.check() is None
    same_bits(a_out.payload.cpu().numpy(), out, "out alone in the arena")

    a_sp = arena((n, k, torch.float32), gpu, poison)
    assert call_bwd(pt, it, order, g_d, ae_d, sl_d, sel_d, a_sp.ptr, n, n, e, D, k) == 0
    torch.cuda.synchronize()
    assert a_sp.check() is None and a_sp.first_poisoned() is None
    same_bits(a_sp.payload.cpu().numpy(), gsp, "grad_sp in the arena")
    cempty = np.diff(structure()[2][0]) == 0
    assert cempty.sum() >= 2 and not mx.bits(gsp[cempty]).any()
    for t, was in zip(ins + [ptr, idx, pt, it, order], keep):
        assert torch.equal(t.view(torch.uint8) if t.dtype == torch.float32 else t,
                           was.view(torch.uint8) if was.dtype == torch.float32 else was)

    # no edges: (+0.0f, -1, 0) and a zero grad_sp; no rows or no columns: nothing is written
    z32 = torch.zeros(n + 1, dtype=torch.int32, device=gpu)
    arenas = [arena((n, D, dt), gpu, poison) for dt in (torch.float32, torch.int32, torch.uint8)]
    a_sp = arena((n, k, torch.float32), gpu, poison)
    assert call_fwd(z32, None, data_d, sel_d, *(a.ptr for a in arenas), n, n, 0, D, k) == 0
    assert call_bwd(z32, None, None, g_d, ae_d, sl_d, sel_d, a_sp.ptr, n, n, 0, D, k) == 0
    torch.cuda.synchronize()
    for a in arenas + [a_sp]:
        assert a.check() is None
    assert not mx.bits(arenas[0].payload.cpu().numpy()).any()
    assert bool((arenas[1].payload == -1).all()) and not bool(arenas[2].payload.any())
    assert not mx.bits(a_sp.payload.cpu().numpy()).any()
    a_out = arena((1, D, torch.float32), gpu, poison)
    assert call_fwd(z32, None, None, None, a_out.ptr, 0, 0, 0, 0, 0, D, k) == 0
    assert call_bwd(z32, None, None, None, None, None, None, a_out.ptr, 0, 0, 0, D, k) == 0
    torch.cuda.synchronize()
    assert bool((a_out.buf == poison).all())
    COVERED.update(names)


# ------------------------------------------------------------------ 7. capture
def test_forward_and_backward_replay_from_one_captured_graph(gpu):
    D, k = 256, 16
    graph = graph_dev(gpu)
    sets = []
    for seed in (1, 2):
        data, sel = mx.tables(NUM, D, k, seed=40 + seed, exact=False)
        g = np.random.default_rng(seed).standard_normal((NUM, D)).astype(np.float32)
        sets.append(tuple(dev_of(a, gpu) for a in (data, sel, g)))

    def step(d, s, g):
        out, ae, sl = fwd(gpu, d, s, D, graph=graph)
        return out, ae, sl, bwd(gpu, g, ae, sl, s, graph=graph)

    eager = [step(*st) for st in sets]
    static = [t.clone() for t in sets[0]]
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):     # one stream-ordered capture, no side streams
        res = step(*static)
    for which in (1, 0, 1):
        for dst, src in zip(static, sets[which]):
            dst.copy_(src)
        res[0].fill_(float("nan")), res[1].fill_(-7), res[2].fill_(99), res[3].fill_(float("nan"))
        cg.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(res, eager[which], ("out", "arg_edge", "arg_slot", "grad_sp")):
            same_bits(got.cpu().numpy(), want.cpu().numpy(), f"replay of input set {which}: {what}")


# ------------------------------------------------------------------ 8. autograd
def csr_graph(gpu):
    ptr, idx = graph_dev(gpu)[:2]
    return mk.CSRGraph(ptr, idx)


def op_aggregate(graph, data, sel, D):
    pt, it, _ = graph.transposed_structure()
    return torch.ops.maxk.max_aggregate(graph.ptr, graph.idx, pt, it, graph.transposed_order(),
                                        data, sel, D)[0]


VIAS = pytest.mark.parametrize("via", ["function", "operator"])


@VIAS
def test_autograd_exact_accumulated_and_views(gpu, via):
    D, k = 256, 16
    data, sel, out, ae, sl = mx.exact_case(D, k)
    g, gsp = exact_backward(D, k)
    data, sel, g = (dev_of(a, gpu) for a in (data, sel, g))
    graph = csr_graph(gpu)
    agg = mk.max_aggregate if via == "function" else op_aggregate
    big = torch.zeros((NUM, k + 3), device=gpu).requires_grad_(True)
    with torch.no_grad():
        big[:, :k] = data
    gs = strided(g, D + 8)
    y = agg(graph, big[:, :k], sel, D)
    same_bits(y.detach().cpu().numpy(), out, "forward")
    y.backward(gs, retain_graph=True)
    same_bits(big.grad[:, :k].cpu().numpy(), gsp, "grad_sp through a view")
    assert not big.grad[:, k:].any()
    y.backward(gs)      # twice through one graph: the gradients accumulate (exactly: x + x)
    same_bits(big.grad[:, :k].cpu().numpy(), 2 * gsp, "accumulated grad_sp")
    d = data.clone().requires_grad_(True)
    (ga,) = torch.autograd.grad((agg(graph, d, sel, D) * g).sum(), d, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiable|once"):
        ga.sum().backward()
    if via == "function":
        o, e, s = mk.max_aggregate(graph, data, sel, D, return_arg=True)
        same_forward((o, e, s), (out, ae, sl), "return_arg")
        assert not e.requires_grad and not s.requires_grad


@VIAS
def test_autograd_launches_only_what_is_needed(gpu, via, monkeypatch):
    D, k = 256, 16
    data, sel, out, ae, sl = mx.exact_case(D, k)
    g, gsp = exact_backward(D, k)
    data, sel, g = (dev_of(a, gpu) for a in (data, sel, g))
    graph = csr_graph(gpu)
    graph.transposed_order()
    agg = mk.max_aggregate if via == "function" else op_aggregate
    fwd_calls, bwd_calls = [], []
    real_f, real_b = ops.max_aggregate_forward, ops.max_aggregate_backward

    def counted_f(ptr, idx, d, s, dim, with_arg=True):
        fwd_calls.append(with_arg)
        return real_f(ptr, idx, d, s, dim, with_arg)

    def counted_b(*a):
        bwd_calls.append(1)
        return real_b(*a)

    monkeypatch.setattr(ops, "max_aggregate_forward", counted_f)
    monkeypatch.setattr(ops, "max_aggregate_backward", counted_b)
    # sp_data needs no gradient: nothing to run backwards, and the Function skips arg_*
    y = agg(graph, data, sel, D)
    assert not y.requires_grad and bwd_calls == []
    same_bits(y.cpu().numpy(), out, "no gradient needed")
    d = data.clone().requires_grad_(True)
    with torch.no_grad():
        y = agg(graph, d, sel, D)
    assert not y.requires_grad
    same_bits(y.cpu().numpy(), out, "no_grad")
    if via == "function":
        assert fwd_calls == [False, False]
    # needed: one forward with arg_*, one backward
    fwd_calls.clear()
    y = agg(graph, d, sel, D)
    assert fwd_calls == [True] and y.requires_grad
    y.backward(g)
    assert bwd_calls == [1]
    same_bits(d.grad.cpu().numpy(), gsp, "grad_sp")
    # an unused output runs nothing
    d = data.clone().requires_grad_(True)
    y = agg(graph, d, sel, D)
    bwd_calls.clear()
    (d.sum() + 0 * y.detach().sum()).backward()
    assert bwd_calls == []


def test_fake_kernels_give_the_shapes(gpu):
    D, k = 256, 16
    data, sel, out, ae, sl = mx.exact_case(D, k)
    graph = csr_graph(gpu)
    pt, it, _ = graph.transposed_structure()
    order = graph.transposed_order()
    real = [dev_of(a, gpu) for a in (data, sel, out, ae, sl)]
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        f = mode.from_tensor
        o, e, s = torch.ops.maxk.max_aggregate(f(graph.ptr), f(graph.idx), f(pt), f(it), f(order),
                                               f(real[0]), f(real[1]), D)
        assert tuple(o.shape) == tuple(e.shape) == tuple(s.shape) == (NUM, D)
        assert (o.dtype, e.dtype, s.dtype) == (torch.float32, torch.int32, torch.uint8)
        gsp = torch.ops.maxk.max_aggregate_backward(f(pt), f(it), f(order), f(real[2]), f(real[3]),
                                                    f(real[4]), f(real[1]))
        assert tuple(gsp.shape) == (NUM, k) and gsp.dtype == torch.float32


def dense_messages64(ptr, idx, X):
    """(out, winner) of max over each row's edges of X[idx[e]] in float64 torch; rows without
    edges are 0."""
    rows = torch.from_numpy(mx.rows_of(ptr))
    n = ptr.size - 1
    msg = X[torch.from_numpy(idx.astype(np.int64))]
    out = torch.full((n, X.shape[1]), -float("inf"), dtype=torch.float64)
    out = out.scatter_reduce(0, rows[:, None].expand_as(msg), msg, "amax", include_self=True)
    return torch.where(torch.isinf(out), torch.zeros_like(out), out)


def test_maxk_max_aggregate_end_to_end(gpu):
    """x -> MaxK -> max aggregation -> x.grad against float64 torch on the densified features.
    Normal inputs: the only ties are between zeros (which carry no gradient to a selected
    feature) and within multi-edges (whose shares add up in the one column)."""
    D, k = 256, 16
    ptr, idx, (pt, _, _) = structure()
    graph = csr_graph(gpu)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((NUM, D)).astype(np.float32)
    g = rng.standard_normal((NUM, D)).astype(np.float32)
    xd = dev_of(x, gpu).requires_grad_(True)
    y = mk.maxk_max_aggregate(xd, graph, k)
    y.backward(dev_of(g, gpu))
    _, sp_index = mk.maxk(xd.detach(), k)
    sel = sp_index.cpu().long()

    def restate(grad):
        x64 = torch.from_numpy(x).double().requires_grad_(True)
        X = torch.zeros_like(x64).scatter(1, sel, x64.gather(1, sel))
        out = dense_messages64(ptr, idx, X)
        out.backward(grad)
        return out.detach(), x64.grad

    ref, gx = restate(torch.from_numpy(g).double())
    _, gmag = restate(torch.from_numpy(np.abs(g)).double())
    same_bits(y.detach().cpu().numpy(), ref.numpy().astype(np.float32), "out")
    # a feature of column c receives at most one term per edge of the column
    bnd = mx.bound(gmag.abs().numpy(), np.diff(pt).astype(np.float64)[:, None])
    err = np.abs(xd.grad.cpu().numpy().astype(np.float64) - gx.numpy())
    assert (err <= bnd).all(), float((err / np.maximum(bnd, 1e-300)).max())
    assert np.count_nonzero(gx.numpy()) > NUM


# ------------------------------------------------------------------ 9. layers
def rel(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).norm() / ref.norm().clamp(min=1e-300))


def masked64(feat64, sel):
    return torch.zeros_like(feat64).scatter(1, sel, feat64.gather(1, sel))


def given_max64(ptr, idx, X, arg_edge):
    """max over each row's edges of X[idx[e]] with the winners given (arg_edge [N, D], -1: the
    implicit zero): a gather, so the gradient goes to the winner alone. Also checks the given
    winners: no candidate of the row beats them by more than rounding."""
    ae = arg_edge.cpu().long()
    col = torch.from_numpy(idx.astype(np.int64))[ae.clamp(min=0)]
    out = torch.where(ae >= 0, X.gather(0, col), torch.zeros_like(X))
    best = dense_messages64(ptr, idx, X.detach())
    assert float((best - out.detach()).abs().max()) <= 1e-5 * float(best.abs().max())
    return out


LAYER_SHAPES = [(64, 64, 8), (256, 128, 32)]


@pytest.mark.parametrize("nonlinear", ["maxk", "relu"])
@pytest.mark.parametrize("fin,fout,k", LAYER_SHAPES)
def test_pool_layer_against_the_dense_float64_restatement(gpu, fin, fout, k, nonlinear):
    ptr, idx, _ = structure()
    graph = csr_graph(gpu)
    torch.manual_seed(fin + k)
    layer = mk.MaxKSAGEConv(fin, fout, "pool", maxk=k, nonlinear=nonlinear).to(gpu)
    with torch.no_grad():
        layer.bias.normal_()
    feat = torch.randn(NUM, fin, device=gpu).requires_grad_(True)
    probe = torch.randn(NUM, fout, device=gpu)
    out = layer(graph, feat)
    (out * probe).sum().backward()
    with pytest.raises(NotImplementedError):
        layer(graph, feat, edge_weight=torch.ones(graph.num_edges, device=gpu))

    p = {n: v.detach().double().cpu().requires_grad_(True) for n, v in layer.named_parameters()}
    f64 = feat.detach().double().cpu().requires_grad_(True)
    with torch.no_grad():       # the selections and winners the layer made, given to the restatement
        if nonlinear == "maxk":
            sp_data, sel1 = mk.maxk(feat.detach(), k)
            x32 = mk.densify(sp_data, sel1, fin)
            pd, sel2 = mk.maxk(layer.fc_pool(x32), k)
            _, ae, _ = mk.max_aggregate(graph, pd, sel2, fin, return_arg=True)
        else:
            h32 = F.relu(layer.fc_pool(feat.detach()))
            sel2 = pooling._identity_selectors(graph, NUM, fin)
            _, ae, _ = mk.max_aggregate(graph, h32, sel2, fin, return_arg=True)
    if nonlinear == "maxk":
        x = masked64(f64, sel1.cpu().long())
        h = masked64(x @ p["fc_pool.weight"].t() + p["fc_pool.bias"], sel2.cpu().long())
    else:
        x = f64
        h = F.relu(x @ p["fc_pool.weight"].t() + p["fc_pool.bias"])
    neigh = given_max64(ptr, idx, h, ae)
    ref = x @ p["fc_self.weight"].t() + neigh @ p["fc_neigh.weight"].t() + p["bias"]
    (ref * probe.double().cpu()).sum().backward()
    assert rel(out, ref) < 1e-5, ("output", rel(out, ref))
    assert rel(feat.grad, f64.grad) < 1e-5, ("feat", rel(feat.grad, f64.grad))
    for name, v in layer.named_parameters():
        assert rel(v.grad, p[name].grad) < 1e-5, (name, rel(v.grad, p[name].grad))


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "edge_weight"])
@pytest.mark.parametrize("nonlinear", ["maxk", "relu"])
@pytest.mark.parametrize("fin,fout,k", LAYER_SHAPES)
def test_gcn_layer_against_the_dense_float64_restatement(gpu, fin, fout, k, nonlinear, weighted):
    ptr, idx, _ = structure()
    graph = csr_graph(gpu)
    torch.manual_seed(fin + k + 1)
    layer = mk.MaxKSAGEConv(fin, fout, "gcn", maxk=k, nonlinear=nonlinear).to(gpu)
    with torch.no_grad():
        layer.bias.normal_()
    feat = torch.randn(NUM, fin, device=gpu).requires_grad_(True)
    probe = torch.randn(NUM, fout, device=gpu)
    ew = (torch.rand(graph.num_edges, device=gpu) + 0.5).requires_grad_(True) if weighted else None
    out = layer(graph, feat, ew)
    (out * probe).sum().backward()

    p = {n: v.detach().double().cpu().requires_grad_(True) for n, v in layer.named_parameters()}
    assert set(p) == {"fc_neigh.weight", "bias"}
    f64 = feat.detach().double().cpu().requires_grad_(True)
    x = f64
    if nonlinear == "maxk":
        x = masked64(f64, mk.maxk(feat.detach(), k)[1].cpu().long())
    rows = torch.from_numpy(mx.rows_of(ptr))
    msg = x[torch.from_numpy(idx.astype(np.int64))]
    w64 = None
    if weighted:
        w64 = ew.detach().double().cpu().requires_grad_(True)
        msg = msg * w64[:, None]
    neigh = torch.zeros_like(x).index_add(0, rows, msg)
    deg = torch.from_numpy(np.diff(ptr).astype(np.float64) + 1)[:, None]
    ref = ((neigh + x) / deg) @ p["fc_neigh.weight"].t() + p["bias"]
    (ref * probe.double().cpu()).sum().backward()
    assert rel(out, ref) < 1e-5, ("output", rel(out, ref))
    assert rel(feat.grad, f64.grad) < 1e-5, ("feat", rel(feat.grad, f64.grad))
    for name, v in layer.named_parameters():
        assert rel(v.grad, p[name].grad) < 1e-5, (name, rel(v.grad, p[name].grad))
    if weighted:
        assert rel(ew.grad, w64.grad) < 1e-5, ("edge_weight", rel(ew.grad, w64.grad))


def test_sage_model_with_the_pool_aggregator_trains_one_step(gpu):
    graph = csr_graph(gpu)
    torch.manual_seed(5)
    model = mk.MaxKSAGE(32, 64, 2, 7, maxk=8, feat_drop=0.2, aggregator_type="pool").to(gpu)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    x = torch.randn(NUM, 32, device=gpu)
    label = torch.randint(0, 7, (NUM,), device=gpu)
    before = [p.detach().clone() for p in model.parameters()]
    loss = F.cross_entropy(model(graph, x), label)
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all())
               for p in model.parameters())
    assert all(float(layer.fc_pool.weight.grad.abs().sum()) > 0 for layer in model.layers)
    opt.step()
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    model.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(model(graph, x)).all())


# ------------------------------------------------------------------ 10. the tile walk
# What the three passes over a tile can get wrong and the 600 x 600 graph does not reach: two hubs
# in one tile (row state 0 and `red` used twice), a tile of short rows alone, a last tile with
# one row, and row counts around one tile. Tie-heavy exact tables, bit for bit.
def walk_graph(which):
    """(ptr, idx, num_cols) of gh.tile_graph ("tile"), gh.tile_graph_t ("tile_t") or
    gh.short_graph(which)."""
    if which == "tile":
        return mx.gh.tile_graph() + (mx.gh.TILE_COLS,)
    if which == "tile_t":
        return mx.gh.tile_graph_t() + (mx.gh.TILE_ROWS,)
    return mx.gh.short_graph(which) + (which,)


@functools.lru_cache(maxsize=None)
def walk_case(which, D, k):
    """(data, sel, out, arg_edge, arg_slot, grad_out, grad_sp) of exact tables on the graph."""
    ptr, idx, nc = walk_graph(which)
    data, sel = mx.tables(nc, D, k, seed=D + k, exact=True)
    out, ae, sl = mx.forward_ref(ptr, idx, data, sel, D)
    g = mx.exact_grad(ptr.size - 1, D, seed=D + k)
    gsp, mag, _ = mx.backward64(ptr, idx, g, ae, sl, sel)
    assert mag.max() * 2 < 2 ** 24          # exactly summable: quanta of 1/2
    return data, sel, out, ae, sl, g, gsp.astype(np.float32)


def walk_dev(which, dev):
    ptr, idx, nc = walk_graph(which)
    return tuple(dev_of(a, dev) for a in (ptr, idx) + mx.transposed(ptr, idx, nc))


def walk_forward(dev, which, D, k):
    data, sel, out, ae, sl, _, _ = walk_case(which, D, k)
    data, sel = dev_of(data, dev), dev_of(sel, dev)
    graph = walk_dev(which, dev)
    same_forward(fwd(dev, data, sel, D, graph=graph), (out, ae, sl), f"{which}")
    alone = fwd(dev, data, sel, D, with_arg=False, graph=graph)[0]
    same_bits(alone.cpu().numpy(), out, f"{which}: out without arg_*")


def walk_backward(dev, which, D, k):
    _, sel, _, ae, sl, g, gsp = walk_case(which, D, k)
    sel, ae, sl, g = (dev_of(a, dev) for a in (sel, ae, sl, g))
    got = bwd(dev, g, ae, sl, sel, graph=walk_dev(which, dev))
    same_bits(got.cpu().numpy(), gsp, f"{which}: grad_sp")


# LP = 8, and LP = 64 with two slots per lane
WALK_SHAPES = [(64, 8), (256, 96)]


@pytest.mark.parametrize("D,k", WALK_SHAPES)
def test_two_hub_rows_share_a_tile(gpu, D, k):
    names = launch_names(k)[:2]
    walk_forward(gpu, "tile", D, k)
    COVERED.update(names)


@pytest.mark.parametrize("D,k", WALK_SHAPES)
def test_two_hub_columns_share_a_tile(gpu, D, k):
    names = launch_names(k)[2:]
    walk_backward(gpu, "tile_t", D, k)
    COVERED.update(names)


@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_row_counts_around_one_tile(gpu, n, D=256, k=16):
    names = launch_names(k)
    walk_forward(gpu, n, D, k)
    walk_backward(gpu, n, D, k)
    COVERED.update(names)


# ------------------------------------------------------------------ 11. closure (keep last)
def test_every_max_instantiation_was_launched_by_a_passing_case(gpu):
    with open(FIXTURE) as f:
        names = {ln.strip() for ln in f if ln.strip()}
    assert len(names) == 12
    missing = sorted(names - COVERED)
    assert not missing, f"instantiations without a passing case: {missing}"
    assert not COVERED - names
