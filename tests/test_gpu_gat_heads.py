"""GPU: the head-batched attention entry points, maxk_heads_aggregate_forward / _backward, their
autograd Functions and operators, and MaxKGATConv(num_heads=H), against the float64 restatements
of tests/gat_heads.py: bit for bit on exactly summable inputs, within the derived bounds of
include/maxk_hip.h ("Multi-head aggregation") on real ones. One 600-row graph serves the module:
its row and column lengths sit on both sides of every limit the library reports and include a
hub row of 5,000 and a hub column of 3,000 edges. The last test closes over the compiled
maxk_mh:: instantiations: each was launched by a passing case that asserted its restated name.

Worst error / bound figures print with -s."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

import gat_heads as gh
import maxk_kernels as mk
from arena import POISONS, arena
from maxk_kernels import _lib, heads, ops

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "kernel_instantiations_heads.txt")
COVERED = set()      # kernel names launched by a case that went on to pass
P = ctypes.c_void_p


def dev_of(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, got.dtype)
    diff = bits(got) != bits(np.asarray(want, np.float32))
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


@functools.lru_cache(maxsize=None)
def structure():
    ptr, idx = gh.graph_arrays()
    return ptr, idx, gh.transposed(ptr, idx, gh.NUM)


def graph_dev(dev):
    ptr, idx, (pt, it, order) = structure()
    return tuple(dev_of(a, dev) for a in (ptr, idx, pt, it, order))


def launch_names(D, H, k):
    """The two instantiations a (D, H, k) call launches, by the restated selectors; checked
    against the fixture before anything runs."""
    names = (gh.fwd_kernel_name(k), gh.bwd_kernel_name(k, H))
    with open(FIXTURE) as f:
        compiled = {ln.strip() for ln in f if ln.strip()}
    assert set(names) <= compiled, names
    return names


def fwd(dev, alpha, data, sel, D, graph=None):
    ptr, idx = (graph or graph_dev(dev))[:2]
    return ops.heads_aggregate(ptr, idx, alpha, data, sel, D)


def bwd(dev, alpha, g, data, sel, need_sp=True, need_alpha=True, graph=None):
    pt, it, order = (graph or graph_dev(dev))[2:]
    return ops.heads_aggregate_backward(pt, it, order, alpha, g, data, sel, need_sp, need_alpha)


def test_limits_are_the_restated_ones(gpu):
    assert ops.heads_row_limits() == gh.LIMITS


# ------------------------------------------------------------------ 1. exact inputs
@functools.lru_cache(maxsize=None)
def exact_case(D, H, k):
    ptr, idx, _ = structure()
    data, sel = gh.tables(gh.NUM, D, k, seed=D + H + k, exact=True)
    alpha = gh.exact_alpha(H, idx.size, seed=k)
    g = gh.exact_grad(gh.NUM, D, seed=H)
    out, mag, _ = gh.forward64(ptr, idx, alpha, data, sel, D)
    (gsp, smag, _), (ga, amag, _) = gh.backward64(ptr, idx, alpha, g, data, sel, D)
    # exactly summable: every partial sum of |terms| stays below 2^23 quanta of 1/8
    assert max(mag.max(), smag.max(), amag.max()) * 8 < 2 ** 23
    return data, sel, alpha, g, out.astype(np.float32), gsp.astype(np.float32), \
        ga.astype(np.float32)


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
EXACT_CASES = [(D, H, k, layout) for D, H, k in gh.SHAPES
               for layout in ("plain", "strided", "records") if layout != "records" or k % 4 == 0]


@pytest.mark.parametrize("D,H,k,layout", EXACT_CASES)
def test_exact_inputs_match_the_restatement_bit_for_bit(gpu, D, H, k, layout):
    names = launch_names(D, H, k)
    data, sel, alpha, g, out, gsp, ga = exact_case(D, H, k)
    data, sel, alpha, g = (dev_of(a, gpu) for a in (data, sel, alpha, g))
    if layout == "strided":
        data, sel, g = strided(data, k + 3), strided(sel, k + 5), strided(g, D + 4)
    elif layout == "records":
        data, sel = records(data, sel)
    got = fwd(gpu, alpha, data, sel, D)
    got_sp, got_a = bwd(gpu, alpha, g, data, sel)
    same_bits(got.cpu().numpy(), out, "out")
    same_bits(got_sp.cpu().numpy(), gsp, "grad_sp")
    same_bits(got_a.cpu().numpy(), ga, "grad_alpha")
    COVERED.update(names)


# ------------------------------------------------------------------ 2. real inputs, 3. attention
@functools.lru_cache(maxsize=None)
def scores(H, seed=4):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((H, gh.NUM)).astype(np.float32),
            rng.standard_normal((H, gh.NUM)).astype(np.float32))


def real_alpha(dev, H):
    ptr, idx = graph_dev(dev)[:2]
    el, er = (dev_of(a, dev) for a in scores(H))
    return ops.gat_attention_heads(ptr, idx, el, er, 0.2)


def worst(err, bnd, lengths, what):
    err, bnd = np.asarray(err, np.float64), np.asarray(bnd, np.float64)
    with np.errstate(all="ignore"):
        ratio = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    reg = np.digitize(np.asarray(lengths), gh.LIMITS[:2], right=True)   # gh.regime, elementwise
    w = [float(ratio[reg == r].max(initial=0.0)) for r in range(3)]
    print(f"\n{what}: worst error / bound per regime {['%.3f' % v for v in w]}")
    assert np.isfinite(ratio).all() and max(w) <= 1.0, (what, w)


@pytest.mark.parametrize("D,H,k", gh.SHAPES)
def test_real_inputs_are_within_the_derived_bounds(gpu, D, H, k):
    names = launch_names(D, H, k)
    ptr, idx, (pt, _, order) = structure()
    data, sel = gh.tables(gh.NUM, D, k, seed=k, exact=False)
    g = np.random.default_rng(H).standard_normal((gh.NUM, D)).astype(np.float32)
    alpha_d = real_alpha(gpu, H)
    alpha = alpha_d.cpu().numpy()
    data_d, sel_d, g_d = (dev_of(a, gpu) for a in (data, sel, g))
    out = fwd(gpu, alpha_d, data_d, sel_d, D).cpu().numpy()
    gsp, ga = (t.cpu().numpy() for t in bwd(gpu, alpha_d, g_d, data_d, sel_d))
    ref, mag, m = gh.forward64(ptr, idx, alpha, data, sel, D)
    (rsp, smag, sm), (ra, amag, am) = gh.backward64(ptr, idx, alpha, g, data, sel, D)
    rlen, clen = np.diff(ptr), np.diff(pt)
    tag = f"(D, H, k) = ({D}, {H}, {k})"
    worst(np.abs(out - ref), gh.bound(mag, m), np.repeat(rlen, D).reshape(-1, D), "out " + tag)
    worst(np.abs(gsp - rsp), gh.bound(smag, sm), np.repeat(clen, k).reshape(-1, k),
          "grad_sp " + tag)
    elen = np.broadcast_to(clen[idx][None, :], ga.shape)   # the regime that served the edge
    worst(np.abs(ga - ra), gh.bound(amag, am), elen, "grad_alpha " + tag)
    assert am.max() <= k and m.max() <= rlen.max() and sm.max() <= clen.max()
    COVERED.update(names)


@pytest.mark.parametrize("H", [1, 3, 8])
def test_batched_attention_is_the_single_head_call_per_head(gpu, H):
    ptr, idx, pt, _, order = graph_dev(gpu)
    el, er = (dev_of(a, gpu) for a in scores(H))
    alpha = ops.gat_attention_heads(ptr, idx, el, er, 0.2)
    ga = dev_of(np.random.default_rng(9).standard_normal(alpha.shape).astype(np.float32), gpu)
    grad_edge, grad_er = ops.gat_attention_backward_heads(ptr, idx, el, er, 0.2, alpha, ga)
    grad_el = ops.edge_colsum_heads(pt, order, grad_edge)
    assert alpha.shape == (H, idx.numel()) and grad_er.shape == grad_el.shape == (H, gh.NUM)
    for h in range(H):
        a1 = ops.gat_attention(ptr, idx, el[h], er[h], 0.2)
        ge1, ger1 = ops.gat_attention_backward(ptr, idx, el[h], er[h], 0.2, a1, ga[h])
        gel1 = ops.edge_colsum(pt, order, ge1)
        for got, want, what in ((alpha[h], a1, "alpha"), (grad_edge[h], ge1, "grad_edge"),
                                (grad_er[h], ger1, "grad_er"), (grad_el[h], gel1, "grad_el")):
            same_bits(got.cpu().numpy(), want.cpu().numpy(), f"{what} head {h} of {H}")
    assert float(grad_el.abs().sum()) > 0
    COVERED.update(gh.ATTENTION_KERNELS)     # the three _heads entry points launch these


def repeat_selectors(sel, seed):
    """In every third column, three slots take the selector of another slot of the column."""
    rng = np.random.default_rng(seed)
    sel = sel.copy()
    k = sel.shape[1]
    for c in range(0, sel.shape[0], 3):
        dst = rng.choice(k, 3, replace=False)
        sel[c, dst] = sel[c, rng.integers(0, k, 3)]
    assert (np.diff(np.sort(sel, axis=1), axis=1) == 0).any(axis=1).sum() >= sel.shape[0] // 6
    return sel


@pytest.mark.parametrize("D,H,k", [(256, 8, 16), (64, 2, 8), (256, 2, 100)])
def test_repeated_nonzero_selectors_are_ordinary_slots(gpu, D, H, k):
    """Slots of one column that name the same feature with nonzero values (not only ref_compat
    padding): their terms add. Exact inputs match the restatement bit for bit; real inputs stay
    within the bound and three calls give the same bits (the forward adds such slots to one LDS
    address in one instruction: include/maxk_hip.h states what that relies on)."""
    ptr, idx, _ = structure()
    data, sel0, alpha, g, _, _, _ = exact_case(D, H, k)
    sel = repeat_selectors(sel0, seed=k)
    out, _, _ = gh.forward64(ptr, idx, alpha, data, sel, D)
    (gsp, _, _), (ga, _, _) = gh.backward64(ptr, idx, alpha, g, data, sel, D)
    d = [dev_of(a, gpu) for a in (alpha, data, sel, g)]
    same_bits(fwd(gpu, d[0], d[1], d[2], D).cpu().numpy(), out.astype(np.float32), "out")
    got_sp, got_a = bwd(gpu, d[0], d[3], d[1], d[2])
    same_bits(got_sp.cpu().numpy(), gsp.astype(np.float32), "grad_sp")
    same_bits(got_a.cpu().numpy(), ga.astype(np.float32), "grad_alpha")

    data, _ = gh.tables(gh.NUM, D, k, seed=k + 7, exact=False)
    g = np.random.default_rng(k).standard_normal((gh.NUM, D)).astype(np.float32)
    alpha_d = real_alpha(gpu, H)
    alpha = alpha_d.cpu().numpy()
    data_d, sel_d, g_d = (dev_of(a, gpu) for a in (data, sel, g))
    runs = [(fwd(gpu, alpha_d, data_d, sel_d, D), *bwd(gpu, alpha_d, g_d, data_d, sel_d))
            for _ in range(3)]
    runs = [[t.cpu().numpy() for t in r] for r in runs]
    for r in runs[1:]:
        for got, first, what in zip(r, runs[0], ("out", "grad_sp", "grad_alpha")):
            same_bits(got, first, what + ", repeated call")
    ref, mag, m = gh.forward64(ptr, idx, alpha, data, sel, D)
    (rsp, smag, sm), (ra, amag, am) = gh.backward64(ptr, idx, alpha, g, data, sel, D)
    for got, r, mg, cnt, what in ((runs[0][0], ref, mag, m, "out"),
                                  (runs[0][1], rsp, smag, sm, "grad_sp"),
                                  (runs[0][2], ra, amag, am, "grad_alpha")):
        err, bnd = np.abs(got - r), gh.bound(mg, cnt)
        assert np.all(err <= bnd), (what, float((err / np.maximum(bnd, 1e-300)).max()))


# ------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("D,H,k", [(256, 8, 16), (96, 3, 10)])
def test_composition_with_the_single_head_path(gpu, D, H, k):
    """Against sum_h spgemm(sp_data * mask_h, sp_index, g, D, edge_weight=alpha[h]) and its
    autograd gradients. The single-head path's bar is the suite's parity bar (oracle.close_enough:
    1e-5 of |ref|, or of sum |terms| where the element cancels); the two paths may differ by the
    sum of that and the new path's derived bound. This checks consistency with the path it
    replaces and no more: the parity bar is about 168 u, far above (m + 4) u for a short row, so
    the accuracy of the new path is held by the exact and the bound tests above, not here."""
    ptr, idx, _ = structure()
    data, sel = gh.tables(gh.NUM, D, k, seed=k + 1, exact=False)
    g = np.random.default_rng(H + 1).standard_normal((gh.NUM, D)).astype(np.float32)
    alpha0 = real_alpha(gpu, H)
    data_d, sel_d, g_d = (dev_of(a, gpu) for a in (data, sel, g))
    graph = mk.CSRGraph(dev_of(ptr, gpu), dev_of(idx, gpu))
    Fh = D // H

    a1, d1 = alpha0.clone().requires_grad_(True), data_d.clone().requires_grad_(True)
    y1 = heads.heads_aggregate(graph, a1, d1, sel_d, D)
    y1.backward(g_d)
    a2, d2 = alpha0.clone().requires_grad_(True), data_d.clone().requires_grad_(True)
    y2 = sum(mk.spgemm(d2 * (sel_d // Fh == h), sel_d, graph, D, edge_weight=a2[h])
             for h in range(H))
    y2.backward(g_d)

    alpha = alpha0.cpu().numpy()
    ref, mag, m = gh.forward64(ptr, idx, alpha, data, sel, D)
    (rsp, smag, sm), (ra, amag, am) = gh.backward64(ptr, idx, alpha, g, data, sel, D)
    for got, other, r, mg, cnt, what in (
            (y1, y2, ref, mag, m, "out"), (d1.grad, d2.grad, rsp, smag, sm, "grad_sp"),
            (a1.grad, a2.grad, ra, amag, am, "grad_alpha")):
        got, other = got.detach().cpu().numpy(), other.detach().cpu().numpy()
        parity = 1e-5 * np.where(np.abs(r) >= 0.5 * mg, np.abs(r), mg)
        tol = gh.bound(mg, cnt) + parity
        err = np.abs(got.astype(np.float64) - other)
        with np.errstate(all="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
        print(f"\ncomposition {what} ({D}, {H}, {k}): worst difference / tolerance "
              f"{ratio.max():.3f}")
        assert ratio.max() <= 1.0, what


# ------------------------------------------------------------------ 5. position, determinism
def moved_graph(picks, lengths, starts, seed):
    """A graph of other size in which the picked segments (lists of column or row indices) are
    rows at other positions, each segment starting at ptr % 4 == its wanted start."""
    rng = np.random.default_rng(seed)
    rows, cols, where = [], [], []
    r = 0
    total = 0
    for seg, start in zip(picks, starts):
        while total % 4 != start:       # filler rows of one edge shift the segment's start
            rows.append(np.array([r])); cols.append(rng.integers(0, gh.NUM, 1)); r += 1; total += 1
        rows.append(np.full(len(seg), r)); cols.append(np.asarray(seg)); where.append(r)
        total += len(seg); r += 1
    n = r + 7
    ptr, idx = gh.csr_from_edges(np.concatenate(rows), np.concatenate(cols), n)
    return ptr, idx, where


def test_rows_and_columns_keep_their_bits_elsewhere(gpu):
    D, H, k = 256, 8, 16
    ptr, idx, (pt, it, order) = structure()
    data, sel = gh.tables(gh.NUM, D, k, seed=21, exact=False)
    alpha_d = real_alpha(gpu, H)
    alpha = alpha_d.cpu().numpy()
    data_d, sel_d = dev_of(data, gpu), dev_of(sel, gpu)
    out = fwd(gpu, alpha_d, data_d, sel_d, D)
    same_bits(fwd(gpu, alpha_d, data_d, sel_d, D).cpu().numpy(), out.cpu().numpy(), "two calls")
    rlen = np.diff(ptr)
    picks = [int(np.argmax(rlen)), int(np.flatnonzero(rlen == 100)[0]),
             int(np.flatnonzero(rlen == 2)[0]), int(np.flatnonzero(rlen == gh.LIMITS[0] + 1)[0])]
    segs = [idx[ptr[r]:ptr[r + 1]] for r in picks]
    ptr2, idx2, where = moved_graph(segs, rlen[picks], (1, 2, 3, 0), seed=5)
    assert [int(ptr2[w]) % 4 for w in where] == [1, 2, 3, 0] and ptr2.size != ptr.size
    alpha2 = np.zeros((H, idx2.size), np.float32)
    alpha2[:] = np.random.default_rng(1).random(alpha2.shape)
    for r, w in zip(picks, where):
        alpha2[:, ptr2[w]:ptr2[w + 1]] = alpha[:, ptr[r]:ptr[r + 1]]
    out2 = ops.heads_aggregate(dev_of(ptr2, gpu), dev_of(idx2, gpu), dev_of(alpha2, gpu), data_d,
                               sel_d, D).cpu().numpy()
    for r, w in zip(picks, where):
        same_bits(out2[w], out.cpu().numpy()[r], f"row {r} of {rlen[r]} edges moved to {w}")

    # columns: the backward on a graph whose transposed structure holds the picked columns
    g = np.random.default_rng(8).standard_normal((gh.NUM, D)).astype(np.float32)
    g_d = dev_of(g, gpu)
    gsp, ga = bwd(gpu, alpha_d, g_d, data_d, sel_d)
    gsp_b, ga_b = bwd(gpu, alpha_d, g_d, data_d, sel_d)
    same_bits(gsp_b.cpu().numpy(), gsp.cpu().numpy(), "grad_sp, two calls")
    same_bits(ga_b.cpu().numpy(), ga.cpu().numpy(), "grad_alpha, two calls")
    clen = np.diff(pt)
    cpicks = [int(np.argmax(clen)), int(np.flatnonzero(clen == 100)[0]),
              int(np.flatnonzero(clen == 2)[0]), int(np.flatnonzero(clen == gh.LIMITS[2] + 1)[0])]
    # transposed structure built by hand: column w of the new structure lists the rows of column
    # c in the same order, its edges carry the same alpha, and its table row is column c's
    rsegs = [it[pt[c]:pt[c + 1]] for c in cpicks]
    pt2, it2, cwhere = moved_graph(rsegs, clen[cpicks], (3, 1, 0, 2), seed=6)
    nc2, e2 = pt2.size - 1, it2.size
    order2 = np.random.default_rng(2).permutation(e2).astype(np.int32)
    alpha2 = np.random.default_rng(3).random((H, e2)).astype(np.float32)
    data2, sel2 = gh.tables(nc2, D, k, seed=22, exact=False)
    for c, w in zip(cpicks, cwhere):
        data2[w], sel2[w] = data[c], sel[c]
        alpha2[:, order2[pt2[w]:pt2[w + 1]]] = alpha[:, order[pt[c]:pt[c + 1]]]
    gsp2, ga2 = ops.heads_aggregate_backward(
        dev_of(pt2, gpu), dev_of(it2, gpu), dev_of(order2, gpu), dev_of(alpha2, gpu), g_d,
        dev_of(data2, gpu), dev_of(sel2, gpu))
    gsp2, ga2, gsp, ga = (t.cpu().numpy() for t in (gsp2, ga2, gsp, ga))
    for c, w in zip(cpicks, cwhere):
        same_bits(gsp2[w], gsp[c], f"column {c} of {clen[c]} edges moved to {w}")
        same_bits(ga2[:, order2[pt2[w]:pt2[w + 1]]], ga[:, order[pt[c]:pt[c + 1]]],
                  f"grad_alpha of column {c}'s edges")


# ------------------------------------------------------------------ 6. non-finite
def test_non_finite_values_stay_in_their_row_column_and_edge(gpu):
    D, H, k = 256, 8, 16
    ptr, idx, (pt, it, order) = structure()
    rows = gh.rows_of(ptr)
    data, sel = gh.tables(gh.NUM, D, k, seed=31, exact=False)
    g = np.random.default_rng(32).standard_normal((gh.NUM, D)).astype(np.float32)
    alpha = real_alpha(gpu, H).cpu().numpy()
    run = lambda a, d: (fwd(gpu, dev_of(a, gpu), dev_of(d, gpu), dev_of(sel, gpu), D).cpu().numpy(),
                        *(t.cpu().numpy() for t in bwd(gpu, dev_of(a, gpu), dev_of(g, gpu),
                                                       dev_of(d, gpu), dev_of(sel, gpu))))
    out0, gsp0, ga0 = run(alpha, data)

    e = int(ptr[np.flatnonzero(np.diff(ptr) == 100)[0]] + 7)    # an edge of a medium row
    bad = alpha.copy()
    bad[2, e], bad[5, e] = np.nan, np.inf
    out, gsp, ga = run(bad, data)
    r, c = rows[e], idx[e]
    assert not np.isfinite(out[r]).all() and not np.isfinite(gsp[c]).all()
    keep_r, keep_c = np.arange(gh.NUM) != r, np.arange(gh.NUM) != c
    same_bits(out[keep_r], out0[keep_r], "rows beside a non-finite alpha")
    same_bits(gsp[keep_c], gsp0[keep_c], "columns beside a non-finite alpha")
    same_bits(ga, ga0, "grad_alpha does not read alpha")

    c = int(np.flatnonzero(np.diff(pt) == 2)[0])                # a column with two edges
    bad = data.copy()
    bad[c, 3] = np.inf
    out, gsp, ga = run(alpha, bad)
    edges = order[pt[c]:pt[c + 1]]
    hit_rows = np.unique(rows[edges])
    keep_r = ~np.isin(np.arange(gh.NUM), hit_rows)
    keep_e = ~np.isin(np.arange(idx.size), edges)
    assert not np.isfinite(out[hit_rows]).all() and not np.isfinite(ga[:, edges]).all()
    same_bits(out[keep_r], out0[keep_r], "rows beside an Inf table value")
    same_bits(ga[:, keep_e], ga0[:, keep_e], "edges beside an Inf table value")
    same_bits(gsp, gsp0, "grad_sp does not read sp_data")


# ------------------------------------------------------------------ 7. output contract
def call_fwd(ptr, idx, alpha, data, sel, out_ptr, H, n, nc, e, D, k):
    return _lib.lib.maxk_heads_aggregate_forward(
        ops._p(ptr), ops._p(idx), ops._p(alpha), ops._p(data), 0, ops._p(sel), 0, P(out_ptr), H,
        n, nc, e, D, k, ops._stream())


def call_bwd(pt, it, order, alpha, g, data, sel, sp_ptr, ga_ptr, H, n, nc, e, D, k):
    return _lib.lib.maxk_heads_aggregate_backward(
        ops._p(pt), ops._p(it), ops._p(order), ops._p(alpha), ops._p(g), 0, ops._p(data), 0,
        ops._p(sel), 0, P(sp_ptr), P(ga_ptr), H, n, nc, e, D, k, ops._stream())


@pytest.mark.parametrize("poison", POISONS)
def test_output_contract(gpu, poison):
    D, H, k = 256, 8, 16
    names = launch_names(D, H, k)
    ptr, idx, pt, it, order = graph_dev(gpu)
    data, sel, alpha, g, out, gsp, ga = exact_case(D, H, k)
    data, sel, alpha, g = (dev_of(a, gpu) for a in (data, sel, alpha, g))
    n, e = gh.NUM, idx.numel()
    a_out = arena((n, D, torch.float32), gpu, poison)
    assert call_fwd(ptr, idx, alpha, data, sel, a_out.ptr, H, n, n, e, D, k) == 0
    torch.cuda.synchronize()
    assert a_out.check() is None and a_out.first_poisoned() is None
    same_bits(a_out.payload.cpu().numpy(), out, "out in the arena")
    empty = np.diff(gh.graph_arrays()[0]) == 0
    assert empty.sum() >= 2 and np.all(bits(a_out.payload.cpu().numpy()[empty]) == 0)

    results = {}
    for want_sp, want_a in ((True, True), (True, False), (False, True), (False, False)):
        a_sp = arena((n, k, torch.float32), gpu, poison)
        a_ga = arena((H, e, torch.float32), gpu, poison)
        rc = call_bwd(pt, it, order, alpha, g, data, sel, a_sp.ptr if want_sp else 0,
                      a_ga.ptr if want_a else 0, H, n, n, e, D, k)
        torch.cuda.synchronize()
        assert rc == 0 and a_sp.check() is None and a_ga.check() is None
        for a, want, ref, what in ((a_sp, want_sp, gsp, "grad_sp"), (a_ga, want_a, ga, "grad_alpha")):
            if want:
                assert a.first_poisoned() is None
                same_bits(a.payload.cpu().numpy(), ref, f"{what} {want_sp, want_a}")
            else:   # untouched
                assert bool((a.buf == poison).all()), what
    cempty = np.diff(structure()[2][0]) == 0
    assert cempty.sum() >= 2 and np.all(bits(gsp[cempty]) == 0)

    # no edges: out and grad_sp are zero-filled; no rows or no columns: nothing is written
    z32 = torch.zeros(n + 1, dtype=torch.int32, device=gpu)
    a_out = arena((n, D, torch.float32), gpu, poison)
    a_sp = arena((n, k, torch.float32), gpu, poison)
    assert call_fwd(z32, None, None, data, sel, a_out.ptr, H, n, n, 0, D, k) == 0
    assert call_bwd(z32, None, None, None, g, data, sel, a_sp.ptr, 0, H, n, n, 0, D, k) == 0
    torch.cuda.synchronize()
    for a in (a_out, a_sp):
        assert a.check() is None and not bits(a.payload.cpu().numpy()).any()
    a_out = arena((1, D, torch.float32), gpu, poison)
    assert call_fwd(z32, None, None, None, None, a_out.ptr, H, 0, 0, 0, D, k) == 0
    assert call_bwd(z32, None, None, None, None, None, None, a_out.ptr, 0, H, 0, 0, 0, D, k) == 0
    torch.cuda.synchronize()
    assert bool((a_out.buf == poison).all())
    COVERED.update(names)


# ------------------------------------------------------------------ 8. capture
def test_forward_and_backward_replay_from_one_captured_graph(gpu):
    D, H, k = 256, 8, 16
    graph = graph_dev(gpu)
    sets = []
    for seed in (1, 2):
        data, sel = gh.tables(gh.NUM, D, k, seed=40 + seed, exact=False)
        rng = np.random.default_rng(seed)
        alpha = rng.random((H, graph[1].numel())).astype(np.float32)
        g = rng.standard_normal((gh.NUM, D)).astype(np.float32)
        sets.append(tuple(dev_of(a, gpu) for a in (alpha, data, sel, g)))
    eager = [(fwd(gpu, a, d, s, D, graph), *bwd(gpu, a, g, d, s, graph=graph))
             for a, d, s, g in sets]
    static = [t.clone() for t in sets[0]]
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):     # one stream-ordered capture, no side streams
        a, d, s, g = static
        res = (fwd(gpu, a, d, s, D, graph), *bwd(gpu, a, g, d, s, graph=graph))
    for which in (1, 0, 1):
        for dst, src in zip(static, sets[which]):
            dst.copy_(src)
        for t in res:
            t.fill_(float("nan"))
        cg.replay()
        torch.cuda.synchronize()
        for got, want, what in zip(res, eager[which], ("out", "grad_sp", "grad_alpha")):
            same_bits(got.cpu().numpy(), want.cpu().numpy(), f"replay of input set {which}: {what}")


# ------------------------------------------------------------------ 9. autograd
def exact_autograd_inputs(gpu, D=256, H=8, k=16):
    data, sel, alpha, g, out, gsp, ga = exact_case(D, H, k)
    return tuple(dev_of(a, gpu) for a in (data, sel, alpha, g)), (out, gsp, ga)


def csr_graph(gpu):
    ptr, idx = graph_dev(gpu)[:2]
    return mk.CSRGraph(ptr, idx)


def op_aggregate(graph, alpha, data, sel, D):
    pt, it, _ = graph.transposed_structure()
    return torch.ops.maxk.heads_aggregate(graph.ptr, graph.idx, pt, it, graph.transposed_order(),
                                          alpha, data, sel, D)


@pytest.mark.parametrize("via", ["function", "operator"])
def test_autograd_exact_twice_accumulated_and_views(gpu, via):
    (data, sel, alpha, g), (out, gsp, ga) = exact_autograd_inputs(gpu)
    graph = csr_graph(gpu)
    agg = heads.heads_aggregate if via == "function" else op_aggregate
    # inputs that are views of larger leaves, an incoming gradient with strided rows
    big_a = torch.zeros((alpha.shape[0] + 2, alpha.shape[1]), device=gpu).requires_grad_(True)
    big_d = torch.zeros((data.shape[0], data.shape[1] + 3), device=gpu).requires_grad_(True)
    with torch.no_grad():
        big_a[1:-1] = alpha
        big_d[:, :data.shape[1]] = data
    gs = strided(g, 256 + 8)
    y = agg(graph, big_a[1:-1], big_d[:, :data.shape[1]], sel, 256)
    same_bits(y.detach().cpu().numpy(), out, "forward")
    y.backward(gs, retain_graph=True)
    same_bits(big_a.grad[1:-1].cpu().numpy(), ga, "grad_alpha through a view")
    same_bits(big_d.grad[:, :data.shape[1]].cpu().numpy(), gsp, "grad_sp through a view")
    assert not big_a.grad[0].any() and not big_d.grad[:, data.shape[1]:].any()
    y.backward(gs)      # twice through one graph: the gradients accumulate (exactly: x + x)
    same_bits(big_a.grad[1:-1].cpu().numpy(), 2 * ga, "accumulated grad_alpha")
    same_bits(big_d.grad[:, :data.shape[1]].cpu().numpy(), 2 * gsp, "accumulated grad_sp")


@pytest.mark.parametrize("via", ["function", "operator"])
def test_autograd_computes_only_the_halves_asked_for(gpu, via, monkeypatch):
    (data, sel, alpha, g), (out, gsp, ga) = exact_autograd_inputs(gpu)
    graph = csr_graph(gpu)
    agg = heads.heads_aggregate if via == "function" else op_aggregate
    calls = []
    real = ops.heads_aggregate_backward

    def counted(*a, need_sp=True, need_alpha=True):
        calls.append((need_sp, need_alpha))
        return real(*a, need_sp=need_sp, need_alpha=need_alpha)

    monkeypatch.setattr(ops, "heads_aggregate_backward", counted)
    for need_a, need_d in ((True, False), (False, True), (False, False)):
        a = alpha.clone().requires_grad_(need_a)
        d = data.clone().requires_grad_(need_d)
        y = agg(graph, a, d, sel, 256)
        calls.clear()
        if not (need_a or need_d):
            assert not y.requires_grad
            continue
        y.backward(g)
        assert calls == [(need_d, need_a)], calls
        if need_a:
            same_bits(a.grad.cpu().numpy(), ga, "grad_alpha alone")
            assert d.grad is None
        else:
            same_bits(d.grad.cpu().numpy(), gsp, "grad_sp alone")
            assert a.grad is None
    # an unused output runs nothing
    a = alpha.clone().requires_grad_(True)
    y = agg(graph, a, data, sel, 256)
    calls.clear()
    (a.sum() + 0 * y.detach().sum()).backward()
    assert calls == []


@pytest.mark.parametrize("via", ["function", "operator"])
def test_autograd_second_order_raises_and_checkpoint_recomputes(gpu, via):
    (data, sel, alpha, g), (out, gsp, ga) = exact_autograd_inputs(gpu)
    graph = csr_graph(gpu)
    agg = heads.heads_aggregate if via == "function" else op_aggregate
    a = alpha.clone().requires_grad_(True)
    y = agg(graph, a, data, sel, 256)
    (ga1,) = torch.autograd.grad((y * g).sum(), a, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiable|once"):
        ga1.sum().backward()
    for reentrant in (False, True):
        a = alpha.clone().requires_grad_(True)
        d = data.clone().requires_grad_(True)
        y = checkpoint(lambda a_, d_: agg(graph, a_, d_, sel, 256), a, d, use_reentrant=reentrant)
        y.backward(g)
        same_bits(a.grad.cpu().numpy(), ga, f"checkpoint reentrant={reentrant}: grad_alpha")
        same_bits(d.grad.cpu().numpy(), gsp, f"checkpoint reentrant={reentrant}: grad_sp")


def attention_case(gpu, H=3):
    """The graph, scores, an incoming gradient and the three kernels' own results for them."""
    graph = csr_graph(gpu)
    pt, order = graph.transposed_structure()[0], graph.transposed_order()
    el0, er0 = (dev_of(a, gpu) for a in scores(H))
    ga = dev_of(np.random.default_rng(9).standard_normal((H, graph.num_edges)).astype(np.float32),
                gpu)
    alpha = ops.gat_attention_heads(graph.ptr, graph.idx, el0, er0, 0.2)
    ge, ger = ops.gat_attention_backward_heads(graph.ptr, graph.idx, el0, er0, 0.2, alpha, ga)
    gel = ops.edge_colsum_heads(pt, order, ge)
    return graph, el0, er0, ga, tuple(t.cpu().numpy() for t in (alpha, gel, ger))


def attention(via, graph, el, er):
    if via == "function":
        return heads.gat_attention_heads(graph, el, er, 0.2)
    return torch.ops.maxk.gat_attention_heads(graph.ptr, graph.idx,
                                              graph.transposed_structure()[0],
                                              graph.transposed_order(), el, er, 0.2)


VIAS = pytest.mark.parametrize("via", ["function", "operator"])


@VIAS
def test_attention_twice_accumulated_views_and_strided_gradient(gpu, via):
    graph, el0, er0, ga, (alpha, gel, ger) = attention_case(gpu)
    H, n = el0.shape
    # inputs that are non-contiguous views of larger leaves, an incoming gradient with strided rows
    big_l = torch.zeros((H, n + 5), device=gpu).requires_grad_(True)
    big_r = torch.zeros((H + 2, n), device=gpu).requires_grad_(True)
    with torch.no_grad():
        big_l[:, 3:3 + n] = el0
        big_r[1:-1] = er0
    y = attention(via, graph, big_l[:, 3:3 + n], big_r[1:-1])
    same_bits(y.detach().cpu().numpy(), alpha, "alpha")
    gs = strided(ga, ga.shape[1] + 7)
    assert not gs.is_contiguous()
    y.backward(gs, retain_graph=True)
    same_bits(big_l.grad[:, 3:3 + n].cpu().numpy(), gel, "grad_el through a view")
    same_bits(big_r.grad[1:-1].cpu().numpy(), ger, "grad_er through a view")
    assert not big_l.grad[:, :3].any() and not big_l.grad[:, 3 + n:].any()
    assert not big_r.grad[0].any() and not big_r.grad[-1].any()
    y.backward(gs)      # twice through one graph: the gradients accumulate (exactly: x + x)
    same_bits(big_l.grad[:, 3:3 + n].cpu().numpy(), 2 * gel, "accumulated grad_el")
    same_bits(big_r.grad[1:-1].cpu().numpy(), 2 * ger, "accumulated grad_er")


@VIAS
def test_attention_runs_only_the_passes_asked_for(gpu, via, monkeypatch):
    """The row pass runs once when either input needs a gradient, the column pass only when el
    does, and nothing is launched when neither does or the output is unused."""
    graph, el0, er0, ga, (alpha, gel, ger) = attention_case(gpu)
    graph.transposed_order()            # built before the counting starts
    calls = []
    real_b, real_c = ops.gat_attention_backward_heads, ops.edge_colsum_heads

    def counted_b(*a, **kw):
        calls.append("rows")
        return real_b(*a, **kw)

    def counted_c(*a, **kw):
        calls.append("columns")
        return real_c(*a, **kw)

    monkeypatch.setattr(ops, "gat_attention_backward_heads", counted_b)
    monkeypatch.setattr(ops, "edge_colsum_heads", counted_c)
    for need_l, need_r, want in ((True, True, ["rows", "columns"]), (False, True, ["rows"]),
                                 (True, False, ["rows", "columns"])):
        el, er = el0.clone().requires_grad_(need_l), er0.clone().requires_grad_(need_r)
        y = attention(via, graph, el, er)
        calls.clear()
        y.backward(ga)
        assert calls == want, (need_l, need_r, calls)
        if need_l:
            same_bits(el.grad.cpu().numpy(), gel, "grad_el")
        else:
            assert el.grad is None
        if need_r:
            same_bits(er.grad.cpu().numpy(), ger, "grad_er")
        else:
            assert er.grad is None
    calls.clear()
    y = attention(via, graph, el0.clone(), er0.clone())
    assert not y.requires_grad and calls == []
    # an unused output: its node is in no path to the loss, nothing is launched
    el, er = el0.clone().requires_grad_(True), er0.clone().requires_grad_(True)
    y = attention(via, graph, el, er)
    (el.sum() + er.sum()).backward()
    assert calls == [] and y.requires_grad
    same_bits(el.grad.cpu().numpy(), np.ones_like(gel), "the other path's gradient")


@VIAS
def test_attention_second_order_raises_and_checkpoint_recomputes(gpu, via):
    graph, el0, er0, ga, (alpha, gel, ger) = attention_case(gpu)
    for which in (0, 1):     # a graph of the backward was asked for: either input's gradient
        el, er = el0.clone().requires_grad_(True), er0.clone().requires_grad_(True)
        y = attention(via, graph, el, er)
        (g1,) = torch.autograd.grad((y * ga).sum(), (el, er)[which], create_graph=True)
        with pytest.raises(RuntimeError, match="differentiable|once"):
            g1.sum().backward()
    for reentrant in (False, True):
        el, er = el0.clone().requires_grad_(True), er0.clone().requires_grad_(True)
        y = checkpoint(lambda l, r: attention(via, graph, l, r), el, er, use_reentrant=reentrant)
        same_bits(y.detach().cpu().numpy(), alpha, f"checkpoint reentrant={reentrant}: alpha")
        y.backward(ga)
        same_bits(el.grad.cpu().numpy(), gel, f"checkpoint reentrant={reentrant}: grad_el")
        same_bits(er.grad.cpu().numpy(), ger, f"checkpoint reentrant={reentrant}: grad_er")


def test_ref_compat_padding_slots_carry_no_gradient(gpu):
    """maxk_heads_aggregate in ref_compat mode on rows that fill fewer than k slots: the padding
    slots (0.0f, 0) pass no gradient into feature 0."""
    D, H, k = 64, 2, 8
    graph = csr_graph(gpu)
    rng = np.random.default_rng(50)
    x = rng.standard_normal((gh.NUM, D)).astype(np.float32)
    x[::3, 5] = 1e6                      # single-hit rows: the pivot leaves padding slots
    x[::3, 0] = -1.0                     # feature 0 is not selected there
    xd = dev_of(x, gpu).requires_grad_(True)
    alpha = dev_of(gh.exact_alpha(H, graph.num_edges, 3), gpu).requires_grad_(True)
    y = heads.maxk_heads_aggregate(xd, graph, alpha, k, mode="ref_compat")
    y.backward(dev_of(gh.exact_grad(gh.NUM, D, 4), gpu))
    sp_data, sp_index, count = ops.maxk_forward(xd.detach(), k, mode="ref_compat",
                                                return_index=True, return_count=True)
    assert int(count.min()) < k
    gx = xd.grad.cpu().numpy()
    short = (count.cpu().numpy() < k) & (x[:, 0] < 0)
    assert short.sum() >= 20 and not gx[short, 0].any()
    assert gx[short, 5].any() and alpha.grad is not None


def test_fake_kernels_give_the_shapes_under_compile(gpu):
    (data, sel, alpha, g), _ = exact_autograd_inputs(gpu)
    graph = csr_graph(gpu)
    pt, it, _ = graph.transposed_structure()
    order = graph.transposed_order()
    el_real = torch.zeros((8, gh.NUM), device=gpu)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(allow_non_fake_inputs=False) as mode:
        f = lambda t: mode.from_tensor(t)
        y = torch.ops.maxk.heads_aggregate(f(graph.ptr), f(graph.idx), f(pt), f(it), f(order),
                                           f(alpha), f(data), f(sel), 256)
        assert tuple(y.shape) == (gh.NUM, 256) and y.dtype == torch.float32
        gsp, ga = torch.ops.maxk.heads_aggregate_backward(f(pt), f(it), f(order), f(alpha), f(g),
                                                          f(data), f(sel), True, False)
        assert tuple(gsp.shape) == tuple(data.shape) and tuple(ga.shape) == (0,)
        el = f(el_real)
        a = torch.ops.maxk.gat_attention_heads(f(graph.ptr), f(graph.idx), f(pt), f(order), el,
                                               el, 0.2)
        assert tuple(a.shape) == (8, graph.num_edges)

    ptr, idx = graph.ptr, graph.idx

    @torch.compile(fullgraph=True, backend="eager")
    def step(alpha, data):
        return torch.ops.maxk.heads_aggregate(ptr, idx, pt, it, order, alpha, data, sel,
                                              256) * 2.0

    want = fwd(gpu, alpha, data, sel, 256) * 2.0
    same_bits(step(alpha, data).cpu().numpy(), want.cpu().numpy(), "compiled, fullgraph")


# ------------------------------------------------------------------ 10. layer
def layer_restatement(layer, graph, feat, sp_index, feat_scale, attn_scale):
    """The layer in float64 torch on the CPU with the selection (sp_index) and the dropout
    scales ([N, k] on the kept values, [H, E] on alpha) given: returns the output and the
    gradients of (out * probe).sum() for every parameter."""
    H, Fo = layer.num_heads, layer.out_feats
    p = {n: v.detach().double().cpu().requires_grad_(True) for n, v in layer.named_parameters()}
    ptr, idx = graph.ptr.cpu().long(), graph.idx.cpu().long()
    rows = torch.repeat_interleave(torch.arange(ptr.numel() - 1), ptr[1:] - ptr[:-1])
    h = feat.double().cpu() @ p["fc.weight"].t()
    hv = h.view(-1, H, Fo)
    el = (hv * p["attn_l"]).sum(-1).t()
    er = (hv * p["attn_r"]).sum(-1).t()
    e = F.leaky_relu(el[:, idx] + er[:, rows], layer.negative_slope)
    m = torch.full((H, ptr.numel() - 1), -float("inf"), dtype=torch.float64)
    m = m.scatter_reduce(1, rows.expand(H, -1), e, "amax")
    ex = torch.exp(e - m[:, rows])
    alpha = ex / torch.zeros_like(m).index_add(1, rows, ex)[:, rows] * attn_scale
    sel = sp_index.cpu().long()
    x = torch.zeros_like(h).scatter(1, sel, h.gather(1, sel) * feat_scale)
    w = alpha.t().repeat_interleave(Fo, dim=1)            # [E, D]: the head's alpha per feature
    out = torch.zeros_like(h).index_add(0, rows, w * x[idx])
    if "bias" in p:
        out = out + p["bias"]
    return out.view(-1, H, Fo), p


def rel(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).norm() / ref.norm().clamp(min=1e-300))


@pytest.mark.parametrize("mode", ["eval", "train", "feat_drop", "feat_drop_fused", "attn_drop"])
@pytest.mark.parametrize("H", [4, 8])
def test_layer_against_the_dense_float64_restatement(gpu, H, mode):
    Fo, k, in_feats = 256 // H, 32, 48
    graph = csr_graph(gpu)
    feat_drop = 0.5 if mode.startswith("feat_drop") else 0.0
    attn_drop = 0.25 if mode == "attn_drop" else 0.0
    torch.manual_seed(H)
    layer = mk.MaxKGATConv(in_feats, Fo, maxk=k, num_heads=H, feat_drop=feat_drop,
                           attn_drop=attn_drop, fused_dropout=mode == "feat_drop_fused",
                           allow_zero_in_degree=True).to(gpu)
    with torch.no_grad():
        layer.bias.normal_()
    assert layer.fc.weight.shape == (H * Fo, in_feats) and layer.attn_l.shape == (H, Fo)
    assert layer.bias.shape == (H * Fo,)
    layer.train(mode != "eval")
    feat = torch.randn(gh.NUM, in_feats, device=gpu)
    probe = torch.randn(gh.NUM, H, Fo, device=gpu)
    torch.manual_seed(77)
    out = layer(graph, feat)
    assert out.shape == (gh.NUM, H, Fo)
    (out * probe).sum().backward()

    # the masks the layer drew, from the same seed in the same order
    torch.manual_seed(77)
    h = layer.fc(feat).detach()
    attn_scale = torch.ones(H, graph.num_edges, dtype=torch.float64)
    feat_scale = torch.ones(gh.NUM, k, dtype=torch.float64)
    if attn_drop:
        attn_scale = F.dropout(torch.ones(H, graph.num_edges, device=gpu), attn_drop,
                               True).double().cpu()
    sp_data, sp_index = mk.maxk(h, k)
    if mode == "feat_drop":
        feat_scale = F.dropout(torch.ones_like(sp_data), feat_drop, True).double().cpu()
    elif mode == "feat_drop_fused":
        seed = torch.empty((), dtype=torch.int64).random_().item()
        dropped, _ = mk.maxk(h, k, dropout_p=feat_drop, training=True, seed=seed)
        feat_scale = (dropped != 0).double().cpu() / (1 - feat_drop)
        assert 0.3 < float((dropped != 0).double().mean()) < 0.7
    ref, p = layer_restatement(layer, graph, feat, sp_index, feat_scale, attn_scale)
    (ref * probe.double().cpu()).sum().backward()
    assert rel(out, ref) < 1e-5, ("output", rel(out, ref))
    for name, v in layer.named_parameters():
        assert rel(v.grad, p[name].grad) < 1e-5, (name, rel(v.grad, p[name].grad))


def test_layer_refusals_and_one_head_unchanged(gpu):
    with pytest.raises(NotImplementedError):
        mk.MaxKGATConv(16, 32, num_heads=2, nonlinear="relu")
    with pytest.raises(ValueError, match="256"):
        mk.MaxKGATConv(16, 64, num_heads=8)
    graph = csr_graph(gpu)
    torch.manual_seed(3)
    layer = mk.MaxKGATConv(48, 64, maxk=16, allow_zero_in_degree=True).to(gpu)
    assert layer.num_heads == 1
    assert {n: tuple(v.shape) for n, v in layer.state_dict().items()} == {
        "fc.weight": (64, 48), "attn_l": (1, 64), "attn_r": (1, 64), "bias": (64,)}
    feat = torch.randn(gh.NUM, 48, device=gpu)
    out = layer(graph, feat)
    # the single-head layer's forward, restated with the single-head entry points
    h = layer.fc(feat)
    el, er = (h * layer.attn_l).sum(-1), (h * layer.attn_r).sum(-1)
    e = F.leaky_relu(el[graph.idx.long()] + er[graph.edge_rows()], 0.2)
    want = mk.maxk_aggregate(h, graph.with_values("sum"), 16, "exact",
                             edge_weight=mk.edge_softmax(graph, e)) + layer.bias
    assert out.shape == (gh.NUM, 64)
    same_bits(out.detach().cpu().numpy(), want.detach().cpu().numpy(), "num_heads=1")


# ------------------------------------------------------------------ 11. the tile walk
# What the three passes over a tile can get wrong and the 600 x 600 graph does not reach: two hubs
# in one tile (row state 0 and `red` used twice), a tile of short rows alone, a last tile with
# one row, and row counts around one tile. Exact inputs, bit for bit.
def walk_graph(which):
    """(ptr, idx, num_cols) of gh.tile_graph ("tile"), gh.tile_graph_t ("tile_t") or
    gh.short_graph(which)."""
    if which == "tile":
        return gh.tile_graph() + (gh.TILE_COLS,)
    if which == "tile_t":
        return gh.tile_graph_t() + (gh.TILE_ROWS,)
    return gh.short_graph(which) + (which,)


@functools.lru_cache(maxsize=None)
def walk_case(which, D, H, k):
    ptr, idx, nc = walk_graph(which)
    data, sel = gh.tables(nc, D, k, seed=D + H + k, exact=True)
    alpha = gh.exact_alpha(H, idx.size, seed=k)
    g = gh.exact_grad(ptr.size - 1, D, seed=H)
    out, mag, _ = gh.forward64(ptr, idx, alpha, data, sel, D)
    (gsp, smag, _), (ga, amag, _) = gh.backward64(ptr, idx, alpha, g, data, sel, D)
    assert max(mag.max(), smag.max(), amag.max()) * 8 < 2 ** 23      # exactly summable
    return data, sel, alpha, g, out.astype(np.float32), gsp.astype(np.float32), \
        ga.astype(np.float32)


def walk_dev(which, dev):
    ptr, idx, nc = walk_graph(which)
    return tuple(dev_of(a, dev) for a in (ptr, idx) + gh.transposed(ptr, idx, nc))


# LP = 8 and LP = 64 with two slots per lane, one head and sixteen (F = 4 at D = 64)
WALK_SHAPES = [(64, 1, 8), (64, 16, 8), (256, 1, 96), (256, 16, 96)]


@pytest.mark.parametrize("D,H,k", WALK_SHAPES)
def test_two_hub_rows_share_a_tile(gpu, D, H, k):
    names = launch_names(D, H, k)
    data, sel, alpha, _, out, _, _ = walk_case("tile", D, H, k)
    data, sel, alpha = (dev_of(a, gpu) for a in (data, sel, alpha))
    got = fwd(gpu, alpha, data, sel, D, graph=walk_dev("tile", gpu))
    same_bits(got.cpu().numpy(), out, "out")
    COVERED.add(names[0])


@pytest.mark.parametrize("D,H,k", WALK_SHAPES)
def test_two_hub_columns_share_a_tile(gpu, D, H, k):
    names = launch_names(D, H, k)
    data, sel, alpha, g, _, gsp, ga = walk_case("tile_t", D, H, k)
    data, sel, alpha, g = (dev_of(a, gpu) for a in (data, sel, alpha, g))
    graph = walk_dev("tile_t", gpu)
    for need_sp, need_alpha in ((True, False), (False, True), (True, True)):
        got_sp, got_a = bwd(gpu, alpha, g, data, sel, need_sp, need_alpha, graph=graph)
        assert (got_sp is None) == (not need_sp) and (got_a is None) == (not need_alpha)
        if need_sp:
            same_bits(got_sp.cpu().numpy(), gsp, f"grad_sp ({need_sp}, {need_alpha})")
        if need_alpha:
            same_bits(got_a.cpu().numpy(), ga, f"grad_alpha ({need_sp}, {need_alpha})")
    COVERED.add(names[1])


@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_row_counts_around_one_tile(gpu, n, H, D=256, k=16):
    names = launch_names(D, H, k)
    data, sel, alpha, g, out, gsp, ga = walk_case(n, D, H, k)
    data, sel, alpha, g = (dev_of(a, gpu) for a in (data, sel, alpha, g))
    graph = walk_dev(n, gpu)
    same_bits(fwd(gpu, alpha, data, sel, D, graph=graph).cpu().numpy(), out, "out")
    for need_sp, need_alpha in ((True, False), (False, True), (True, True)):
        got_sp, got_a = bwd(gpu, alpha, g, data, sel, need_sp, need_alpha, graph=graph)
        assert (got_sp is None) == (not need_sp) and (got_a is None) == (not need_alpha)
        if need_sp:
            same_bits(got_sp.cpu().numpy(), gsp, f"grad_sp ({need_sp}, {need_alpha})")
        if need_alpha:
            same_bits(got_a.cpu().numpy(), ga, f"grad_alpha ({need_sp}, {need_alpha})")
    COVERED.update(names)


# ------------------------------------------------------------------ 12. closure (keep last)
def test_every_heads_instantiation_was_launched_by_a_passing_case(gpu):
    with open(FIXTURE) as f:
        names = {ln.strip() for ln in f if ln.strip()}
    assert len(names) == 14
    missing = sorted(names - COVERED)
    assert not missing, f"instantiations without a passing case: {missing}"
    assert not COVERED - names
