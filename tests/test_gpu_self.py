"""GPU: the self-term path. The MaxK top-k also emits the dense masked row
(maxk_topk_cbsr_dense) and its scatter adds the dense row's gradient (maxk_scatter_backward_merge),
through the C ABI's Python binding, maxk_self_aggregate, the layers and the torch operators.

Both kernels are held bit for bit to the numpy restatement of test_self_capi.py (dense_rows,
merge_rows) applied to the tables of the existing entry points, which test_gpu_parity,
test_gpu_records and test_gpu_dropout pin to the oracle and to the numpy mask."""
import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import maxk_kernels as mk
from maxk_kernels import graphs, layers, ops
from maxk_kernels.layers import MaxKGIN, MaxKGINConv, MaxKSAGE, MaxKSAGEConv
from oracle import oracle
from test_dropout_capi import drop_scale, dropped_table, keep_mask
from test_gpu_dropout import CASES_67, D_E2E, N_E2E, SEED, _drawn_seed, _mask64, bits
from test_gpu_dropout import e2e_graph  # noqa: F401  (module-scoped fixture)
from test_gpu_parity import assert_close, graph_on
from test_gpu_records import MODES, SENTINEL, chunk_bytes, special_rows
from test_layers import close, dense_adj, maxk_dense, small_edges
from test_self_capi import dense_rows, merge_rows

pytestmark = pytest.mark.gpu


def topk(x, k, mode, p, layout=None, stats=True, dense=None, row_offset=0, values=True):
    """One top-k launch with every output: (sd, si, cnt, rec, st)."""
    n = x.shape[0]
    st = torch.full((2,), -1, dtype=torch.int32, device=x.device) if stats else None
    rec = None
    if layout is not None:
        rec = torch.full((n, chunk_bytes(layout, k) + 16), SENTINEL, dtype=torch.uint8,
                         device=x.device)
    sd, si, cnt = mk.maxk_forward(x, k, mode=mode, return_index=True, return_count=True,
                                  records=None if rec is None else (rec, layout), stats=st,
                                  dropout=(p, SEED, row_offset), dense=dense,
                                  return_values=values)
    return sd, si, cnt, rec, st


def check_dense(x, k, mode, p, layout=None, row_offset=0):
    """The dense launch against dense_rows of the existing entry point's table; every other
    output bit-identical to the launch without ``dense``; and ``dense`` alone."""
    n, d = x.shape
    sd0, si0, cnt0, rec0, st0 = topk(x, k, mode, p, layout, row_offset=row_offset)
    want = dense_rows(sd0.cpu().numpy(), si0.cpu().numpy(), cnt0.cpu().numpy(), d)
    dense = torch.full((n, d), float("nan"), device=x.device)
    sd, si, cnt, rec, st = topk(x, k, mode, p, layout, dense=dense, row_offset=row_offset)
    assert torch.equal(bits(dense), bits(want)), (k, mode, p, layout)
    assert torch.equal(bits(sd), bits(sd0)) and torch.equal(si, si0) and torch.equal(cnt, cnt0)
    assert st.tolist() == st0.tolist()
    if layout is not None:
        assert torch.equal(rec, rec0)
    # neither records nor a value table: dense is the only value output
    alone = torch.full((n, d), float("nan"), device=x.device)
    sd, si, cnt, _, _ = topk(x, k, mode, p, None, stats=False, dense=alone,
                             row_offset=row_offset, values=False)
    assert sd is None and torch.equal(si, si0) and torch.equal(cnt, cnt0)
    assert torch.equal(bits(alone), bits(want))
    return dense, sd0, si0, cnt0


# ------------------------------------------------------------------ dense top-k
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("mode", MODES)
def test_dense_topk_bit_exact(gpu, mode, p):
    """N = 67: no multiple of the rows per wave or work-group; D = 256: the full-row kernels;
    k = 128: the k > 64 kernels; layout None: no records."""
    for layout, k in CASES_67:
        x = graphs.features(67, 256, seed=100 + k).to(gpu)
        dense, sd0, _, cnt0 = check_dense(x, k, mode, p, layout=layout)
        if p > 0:           # among the filled slots something is dropped and something kept
            filled = torch.arange(k)[None, :] < cnt0.cpu()[:, None]
            kept = (bits(sd0) != 0)[filled]
            assert 0.3 < float(kept.float().mean()) < 0.9, (layout, k)
        assert int((bits(dense) != 0).sum()) == int((bits(sd0) != 0).sum()), (layout, k)


@pytest.mark.parametrize("mode", MODES)
def test_dense_topk_partial_rows(gpu, mode):
    """D = 100 (partial-row masks) and D = 99 (scalar loads and stores) at n = 5."""
    for d, k in ((100, 8), (99, 10)):
        x = graphs.features(5, d, seed=35 + d).to(gpu)
        for p in (0.0, 0.5):
            for layout in (None, 2, 4):
                check_dense(x, k, mode, p, layout=layout)


@pytest.mark.parametrize("mode", MODES)
def test_dense_topk_row_stride_leaves_the_gap(gpu, mode):
    for d, k in ((256, 16), (100, 8), (99, 10)):
        n = 21
        x = graphs.features(n, d, seed=d + k).to(gpu)
        for p in (0.0, 0.5):
            sd0, si0, cnt0, _, _ = topk(x, k, mode, p)
            want = dense_rows(sd0.cpu().numpy(), si0.cpu().numpy(), cnt0.cpu().numpy(), d)
            buf = torch.full((n, d + 12), -7.0, device=gpu)
            view = buf[:, :d]
            assert view.stride(0) == d + 12 and not view.is_contiguous()
            topk(x, k, mode, p, 4, dense=view)
            assert torch.equal(bits(view), bits(want))
            assert bool((buf[:, d:] == -7.0).all()), "floats between the rows were written"


@pytest.mark.parametrize("mode", MODES)
def test_dense_topk_rows_that_are_not_16_byte_aligned(gpu, mode):
    """A base one float into a buffer, and a row stride of D + 1: scalar stores, same rows."""
    n, d, k = 21, 256, 16
    x = graphs.features(n, d, seed=5).to(gpu)
    for p in (0.0, 0.5):
        sd0, si0, cnt0, _, _ = topk(x, k, mode, p)
        want = dense_rows(sd0.cpu().numpy(), si0.cpu().numpy(), cnt0.cpu().numpy(), d)
        for width, first in ((d + 4, 1), (d + 1, 0)):
            buf = torch.full((n, width), -7.0, device=gpu)
            view = buf[:, first:first + d]
            assert view.data_ptr() % 16 != 0 or view.stride(0) % 4 != 0
            topk(x, k, mode, p, 4, dense=view)
            assert torch.equal(bits(view), bits(want))
            assert bool((buf[:, :first] == -7.0).all()) and bool((buf[:, first + d:] == -7.0).all())


@pytest.mark.parametrize("k", [16, 66])
@pytest.mark.parametrize("mode", MODES)
def test_dense_topk_special_rows(gpu, k, mode):
    """NaN, Inf, denormals, all-equal and single-spike rows: dropped slots and unselected
    features are +0.0f exactly; a selected -0.0f keeps its sign."""
    x = special_rows(256, seed=k)
    x[9, :] = -1.0                       # row 9: 4 ones, then -0.0f: exact mode selects the
    x[9, :4] = 1.0                       # ones and the first k - 4 of the -0.0f (ties low)
    x[9, 4:4 + 2 * k] = -0.0
    x = x.to(gpu)
    for p in (0.0, 0.5):
        dense, sd0, si0, cnt0 = check_dense(x, k, mode, p, layout=4)
        db = bits(dense)
        filled = torch.arange(k)[None, :] < cnt0.cpu()[:, None]
        selected = torch.zeros((12, 256), dtype=torch.bool)
        selected[torch.arange(12)[:, None].expand(12, k)[filled], si0.cpu().long()[filled]] = True
        assert bool((db[~selected] == 0).all())
        if p > 0:
            keep = torch.from_numpy(keep_mask(p, SEED, np.arange(12)[:, None],
                                              np.arange(256)[None, :]))
            assert bool((db[selected & ~keep] == 0).all())
    if mode == "exact":
        d0 = torch.full((12, 256), float("nan"), device=gpu)
        topk(x, k, mode, 0.0, dense=d0)
        row = bits(d0)[9]
        assert int((row == -2 ** 31).sum()) == k - 4 and bool((row[4:k] == -2 ** 31).all())


def test_dense_topk_ref_compat_padding_leaves_feature_0(gpu):
    """Single-hit rows: the padding slots name selector 0, feature 0 stays +0.0f; and rows
    with more than k entries above the threshold keep only the first k."""
    x = graphs.features(67, 256, seed=77)
    x[::7, 5] = 1e6
    x[3, :] = 0.0
    x[3, 10:60] = 1.0                    # 50 entries tie above p: only the first k are emitted
    x = x.to(gpu)
    for p in (0.5, 0.0):
        dense, sd0, si0, cnt0 = check_dense(x, 16, "ref_compat", p, layout=4)
        assert cnt0[::7].tolist() == [1] * len(cnt0[::7]) and int(cnt0[3]) == 16
        assert bool((bits(dense)[::7, 0] == 0).all())
        assert bool((bits(dense)[::7, :5] == 0).all()) and bool((bits(dense)[::7, 6:] == 0).all())
        assert bool((bits(dense)[3, 26:] == 0).all())
    assert bool((dense[::7, 5] == 1e6).all())


@pytest.mark.parametrize("mode", MODES)
def test_dense_topk_row_offset(gpu, mode):
    x = graphs.features(67, 256, seed=9).to(gpu)
    full = torch.empty_like(x)
    topk(x, 16, mode, 0.5, dense=full)
    part = torch.empty((30, 256), device=gpu)
    topk(x[20:50].contiguous(), 16, mode, 0.5, dense=part, row_offset=20)
    assert torch.equal(bits(part), bits(full[20:50]))
    check_dense(x[20:50].contiguous(), 16, mode, 0.5, layout=4, row_offset=20)


def test_dense_argument_checks(gpu):
    x = graphs.features(8, 64, seed=1).to(gpu)
    with pytest.raises(RuntimeError, match="dense must be"):
        mk.maxk_forward(x, 8, dense=torch.empty((8, 60), device=gpu))
    with pytest.raises(RuntimeError, match="float32"):
        mk.maxk_forward(x, 8, dense=torch.empty((8, 64), device=gpu, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="overlaps"):
        mk.maxk_forward(x, 8, dense=x)
    with pytest.raises(RuntimeError, match="needs records"):
        mk.maxk_forward(x, 8, return_values=False)


# ------------------------------------------------------------------ merge scatter
def _merge_inputs(n, d, k, seed):
    x = graphs.features(n, d, seed=11 + seed)
    _, oi = oracle.maxk(x.numpy(), k)
    return oi, graphs.features(n, k, seed=12 + seed), graphs.features(n, d, seed=13 + seed)


@pytest.mark.parametrize("d,k", [(256, 16), (256, 128), (100, 16), (99, 10)])
def test_merge_scatter_bit_exact(gpu, d, k):
    n = 67
    oi, g, gd = _merge_inputs(n, d, k, k)
    gi, gg, gdg = torch.from_numpy(oi).to(gpu), g.to(gpu), gd.to(gpu)
    for p, seed, off in ((0.0, SEED, 0), (0.25, 3, 1000), (0.5, SEED, 0), (1.0, SEED, 0)):
        drop = (p, seed, off)
        want = merge_rows(g.numpy(), oi, gd.numpy(), p, seed, off)
        got = mk.maxk_backward(gg, gi, dim_origin=d, dropout=drop, grad_dense=gdg)
        assert torch.equal(bits(got), bits(want)), (p, "both")
        # only the dense output was used
        want = merge_rows(None, oi, gd.numpy(), p, seed, off)
        got = mk.maxk_backward(None, gi, dim_origin=d, dropout=drop, grad_dense=gdg)
        assert torch.equal(bits(got), bits(want)), (p, "dense alone")
        # without grad_dense: today's call; the merge entry point agrees with it bit for bit
        today = mk.maxk_backward(gg, gi, dim_origin=d, dropout=drop)
        assert torch.equal(bits(today), bits(merge_rows(g.numpy(), oi, None, p, seed, off, D=d)))
        got = torch.empty_like(today)
        ops.check(ops.lib.maxk_scatter_backward_merge(ops._p(gg), ops._p(gi), 0, None, 0,
                                                      ops._p(got), n, d, k, p, seed, off,
                                                      ops._stream()), "merge")
        assert torch.equal(bits(got), bits(today)), (p, "sparse alone")
    # a row-strided grad_dense
    buf = torch.full((n, d + 12), float("nan"), device=gpu)
    buf[:, :d] = gdg
    got = mk.maxk_backward(gg, gi, dim_origin=d, dropout=(0.5, SEED), grad_dense=buf[:, :d])
    assert torch.equal(bits(got), bits(merge_rows(g.numpy(), oi, gd.numpy(), 0.5, SEED)))
    with pytest.raises(RuntimeError, match="needs grad_dense"):
        mk.maxk_backward(None, gi, dim_origin=d)
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.check(ops.lib.maxk_scatter_backward_merge(ops._p(gg), ops._p(gi), 0, ops._p(gdg), 0,
                                                      ops._p(gdg), n, d, k, 0.0, 0, 0,
                                                      ops._stream()), "merge")


def test_merge_scatter_repeated_selectors(gpu):
    """The last slot still wins, with that feature's dense gradient and mask."""
    n, d, k = 9, 64, 8
    oi = np.random.default_rng(4).integers(0, 6, size=(n, k)).astype(np.uint8)
    g, gd = graphs.features(n, k, seed=2), graphs.features(n, d, seed=3)
    for p in (0.0, 0.5):
        got = mk.maxk_backward(g.to(gpu), torch.from_numpy(oi).to(gpu), dim_origin=d,
                               dropout=(p, SEED), grad_dense=gd.to(gpu))
        assert torch.equal(bits(got), bits(merge_rows(g.numpy(), oi, gd.numpy(), p, SEED)))


def test_merge_scatter_strided_selectors_and_non_finite_dense(gpu):
    """The selector view of layout-1 records (row-strided u8); NaN / Inf in grad_dense at
    unselected features do not leak: those features are +0.0f."""
    n, d, k = 67, 256, 16
    oi, g, gd = _merge_inputs(n, d, k, 5)
    selected = np.zeros((n, d), bool)
    selected[np.arange(n)[:, None], oi] = True
    gd = gd.numpy().copy()
    gd[~selected] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), (~selected).sum())
    rec = torch.full((n, 128), SENTINEL, dtype=torch.uint8, device=gpu)
    rec[:, 4 * k:5 * k] = torch.from_numpy(oi).to(gpu)
    sel = rec[:, 4 * k:5 * k]
    assert sel.stride(0) == 128 and not sel.is_contiguous()
    for p in (0.0, 0.5):
        got = mk.maxk_backward(g.to(gpu), sel, dim_origin=d, dropout=(p, SEED),
                               grad_dense=torch.from_numpy(gd).to(gpu))
        assert torch.equal(bits(got), bits(merge_rows(g.numpy(), oi, gd, p, SEED)))
        assert bool((bits(got)[torch.from_numpy(~selected)] == 0).all())
        assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------ end to end
def _filled_count(od, oi):
    """Filled slots per row of an undropped ref_compat oracle table: selectors ascend, so a slot
    past the first that names feature 0 is padding; slot 0 is filled when it is not (0.0f, 0)
    or slot 1 is filled. (A filled slot 0 that holds x[r, 0] == 0.0f would read as padding: the
    inputs here have none.) A constant row fills nothing: count 0."""
    later = (oi[:, 1:] != 0).sum(1)
    first = (od[:, 0] != 0) | (oi[:, 0] != 0) | (later > 0)
    return later + first


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("k", [8, 16, 32])
@pytest.mark.parametrize("mode", MODES)
def test_maxk_self_aggregate_end_to_end(gpu, e2e_graph, k, mode, p_drop):  # noqa: F811
    p, ix, v = e2e_graph
    n, d = N_E2E, D_E2E
    x = graphs.features(n, d, seed=31 + k)
    x[::7, 5] = 1e6                          # ref_compat: single-hit rows with padding slots
    x[11, :] = 0.5                           # constant rows: ref_compat fills no slot (lo == hi,
    x[18, :] = 0.0                           # nothing above p), so the row passes no gradient
    g_agg = graphs.features(n, d, seed=32 + k)
    g_self = graphs.features(n, d, seed=33 + k)
    graph = mk.CSRGraph(*graph_on(gpu, p, ix, v))
    layout = graph.plan(d, k).info()["fwd_layout"]
    if k == 16:
        assert layout == 4
    if k == 8:
        assert layout == 2

    od, oi = oracle.maxk(x.numpy(), k, mode)
    odd = dropped_table(od, oi, p_drop, SEED) if p_drop else od
    cnt = _filled_count(od, oi) if mode == "ref_compat" else None
    if cnt is not None:
        assert cnt[11] == 0 and cnt[18] == 0 and cnt[0] == 1
    xm_ref = dense_rows(odd, oi, cnt, d)
    ref, mag = oracle.spgemm_forward(p, ix, v, odd, oi, d, with_mag=True)
    gs, gmag = oracle.sspmm_backward(p, ix, v, g_agg.numpy(), oi, with_mag=True)
    scale = float(drop_scale(p_drop)) if p_drop else 1.0
    keep = keep_mask(p_drop, SEED, np.arange(n)[:, None], oi) if p_drop else np.ones_like(oi, bool)
    filled = (np.arange(k)[None, :] < cnt[:, None]) if cnt is not None else np.ones_like(od, bool)
    rows = np.repeat(np.arange(n)[:, None], k, 1)

    def scattered(vals):
        out = np.zeros((n, d))
        out[rows[filled], oi[filled]] = vals[filled]
        return out

    gself_k = np.take_along_axis(g_self.numpy().astype(np.float64), oi.astype(np.int64), 1)
    both = scattered((gs.astype(np.float64) + gself_k) * keep * scale)
    both_mag = scattered((gmag.astype(np.float64) + np.abs(gself_k)) * scale)
    only_agg = scattered(gs.astype(np.float64) * keep * scale)
    only_agg_mag = scattered(gmag.astype(np.float64) * scale)
    only_self = scattered(gself_k * keep * scale)
    only_self_mag = scattered(np.abs(gself_k) * scale)

    def run(gs_, ga_):
        xg = x.to(gpu).requires_grad_(True)
        xm, y = mk.maxk_self_aggregate(xg, graph, k, mode, dropout_p=p_drop, seed=SEED)
        outs = [t for t, g in ((xm, gs_), (y, ga_)) if g is not None]
        torch.autograd.backward(outs, [g.to(gpu) for g in (gs_, ga_) if g is not None])
        return xm, y, xg.grad

    xm, y, gx = run(g_self, g_agg)
    assert torch.equal(bits(xm), bits(xm_ref))
    if mode == "ref_compat":                 # the empty rows: nothing out, nothing back
        assert not both[[11, 18]].any() and not only_self[[11, 18]].any()
        assert bool((bits(xm)[[11, 18]] == 0).all()) and bool((bits(gx)[[11, 18]] == 0).all())
        assert float(g_self[11, 0]) != 0 and float(g_self[18, 0]) != 0
    assert_close(y, ref, mag)
    assert_close(gx, both, both_mag)
    assert_close(run(None, g_agg)[2], only_agg, only_agg_mag)
    assert_close(run(g_self, None)[2], only_self, only_self_mag)
    # same records, same forward as maxk_aggregate
    y2 = mk.maxk_aggregate(x.to(gpu), graph, k, mode, dropout_p=p_drop, seed=SEED)
    assert torch.equal(y, y2)
    # an unused pair gives no gradient and no launch
    xg = x.to(gpu).requires_grad_(True)
    xm, y = mk.maxk_self_aggregate(xg, graph, k, mode)
    (xg * 2).sum().backward()
    assert bool((xg.grad == 2).all())


def test_self_aggregate_runs_no_pack_or_statistics_pass(gpu, e2e_graph, monkeypatch):  # noqa: F811
    p, ix, v = e2e_graph
    graph = mk.CSRGraph(*graph_on(gpu, p, ix, v))
    assert graph.plan(D_E2E, 16).new_records() is not None

    def boom(*a, **kw):
        raise AssertionError("the per-call pack / statistics path was taken")

    monkeypatch.setattr(ops.GraphPlan, "forward", boom)
    monkeypatch.setattr(ops, "cbsr_stats", boom)
    x = graphs.features(N_E2E, D_E2E, seed=3).to(gpu).requires_grad_(True)
    for p_drop in (0.0, 0.5):
        xm, y = mk.maxk_self_aggregate(x, graph, 16, dropout_p=p_drop, seed=SEED)
        (xm.sum() + y.sum()).backward()
    assert bool(torch.isfinite(x.grad).all())


# ------------------------------------------------------------------ layers
def _spy(monkeypatch):
    calls = []
    real = layers.maxk_self_aggregate

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(layers, "maxk_self_aggregate", spy)
    return calls


@pytest.mark.parametrize("case", ["no_drop", "eval", "fused", "composition"])
@pytest.mark.parametrize("kind", ["sage", "gin"])
def test_self_term_layers_match_dense(gpu, kind, case, monkeypatch):
    dst, src, n = small_edges()
    csr = mk.CSRGraph.from_edges(src.to(gpu), dst.to(gpu), n)
    k, d = 16, 64
    p = 0.0 if case == "no_drop" else 0.5
    fused = case == "fused"
    torch.manual_seed(0)
    if kind == "sage":
        conv = MaxKSAGEConv(d, 48, "mean", feat_drop=p, maxk=k, fused_dropout=fused).to(gpu)
    else:
        conv = MaxKGINConv(d, maxk=k, feat_drop=p, fused_dropout=fused).to(gpu)
    conv.train(case != "eval")
    calls = _spy(monkeypatch)
    x = graphs.features(n, d, seed=3).to(gpu).requires_grad_(True)
    w = graphs.features(n, 48 if kind == "sage" else d, seed=4).to(gpu)
    seed = _drawn_seed(17)
    y = conv(csr, x)
    (y * w).sum().backward()
    assert len(calls) == (0 if case == "composition" else 1)
    if case == "composition":      # F.dropout's own random numbers: nothing to compare against
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all())
        return

    M = _mask64(p, seed, n, d) if case == "fused" else 1.0
    xr = x.detach().cpu().double().requires_grad_(True)
    P = {name: t.detach().cpu().double() for name, t in conv.named_parameters()}
    xm = maxk_dense(xr, k) * M
    if kind == "sage":
        yr = xm @ P["fc_self.weight"].T + (dense_adj(csr, "mean") @ xm) @ P["fc_neigh.weight"].T \
            + P["bias"]
    else:
        yr = (1 + P["eps"]) * xm + dense_adj(csr, "sum") @ xm
    (yr * w.cpu().double()).sum().backward()
    assert close(y, yr), float((y.detach().double().cpu() - yr).abs().max())
    assert close(x.grad, xr.grad)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("model_cls", [MaxKSAGE, MaxKGIN])
def test_self_term_models_train(gpu, model_cls, fused, monkeypatch):
    """test_layers.test_model_trains (same graph, sizes, feat_drop); a short run."""
    dst, src, n = small_edges(n=800, e=16000, seed=11)
    csr = mk.CSRGraph.from_edges(src.to(gpu), dst.to(gpu), n)
    torch.manual_seed(3)
    feats = graphs.features(n, 32, seed=12).to(gpu)
    labels = torch.randint(0, 5, (n,), generator=torch.Generator().manual_seed(1)).to(gpu)
    model = model_cls(32, 64, 2, 5, maxk=16, feat_drop=0.1, norm=True, fused_dropout=fused).to(gpu)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    calls = _spy(monkeypatch)
    losses = []
    for _ in range(12):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(csr, feats), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert len(calls) == (24 if fused else 0)
    with torch.no_grad():
        model.eval()(csr, feats)
    assert len(calls) == (26 if fused else 2)


# ------------------------------------------------------------------ torch operators
def test_torch_ops_self(gpu):
    n, d, k = 300, 64, 16
    seed = -1234567890123456789                      # int64 schema int, read as uint64
    x0 = graphs.features(n, d, seed=1).to(gpu)
    g = graphs.features(n, k, seed=2).to(gpu)
    gd = graphs.features(n, d, seed=3).to(gpu)
    for p in (0.0, 0.5):
        dn, sd, si = torch.ops.maxk.maxk_dense_forward(x0, k, p, seed)
        want = torch.empty_like(x0)
        ed, ei = mk.maxk_forward(x0, k, return_index=True, dropout=(p, seed), dense=want)
        assert torch.equal(bits(dn), bits(want)) and torch.equal(bits(sd), bits(ed))
        assert torch.equal(si, ei)
        gx = torch.ops.maxk.maxk_merge_backward(g, si, gd, p, seed)
        assert torch.equal(bits(gx), bits(mk.maxk_backward(g, si, d, dropout=(p, seed),
                                                           grad_dense=gd)))
    with FakeTensorMode():
        fake = torch.empty((n, d), device="cuda")
        outs = torch.ops.maxk.maxk_dense_forward(fake, k, 0.5, seed)
        assert [tuple(t.shape) for t in outs] == [(n, d), (n, k), (n, k)]
        assert [t.dtype for t in outs] == [torch.float32, torch.float32, torch.uint8]
        out = torch.ops.maxk.maxk_merge_backward(outs[1], outs[2], fake, 0.5, seed)
        assert tuple(out.shape) == (n, d) and out.dtype == torch.float32
    torch.library.opcheck(torch.ops.maxk.maxk_dense_forward.default, (x0, k, 0.5, seed))
    torch.library.opcheck(torch.ops.maxk.maxk_merge_backward.default, (g, si, gd, 0.5, seed))

    def step(x):
        dense, data, _ = torch.ops.maxk.maxk_dense_forward(x, k, 0.5, seed)
        return (data * g).sum() + (dense * gd).sum()

    gx = torch.ops.maxk.maxk_merge_backward(g, si, gd, 0.5, seed)
    xe = x0.clone().requires_grad_(True)
    step(xe).backward()
    assert torch.equal(bits(xe.grad), bits(gx))      # the registered derivative
    # only the dense output used: no [N, k] gradient is made up
    g1 = torch.ops.maxk.maxk_merge_backward(None, si, gd, 0.5, seed)
    assert torch.equal(bits(g1), bits(mk.maxk_backward(None, si, d, dropout=(0.5, seed),
                                                       grad_dense=gd)))
    torch.library.opcheck(torch.ops.maxk.maxk_merge_backward.default, (None, si, gd, 0.5, seed))
    xe = x0.clone().requires_grad_(True)
    (torch.ops.maxk.maxk_dense_forward(xe, k, 0.5, seed)[0] * gd).sum().backward()
    assert torch.equal(bits(xe.grad), bits(g1))
    xe = x0.clone().requires_grad_(True)
    (torch.ops.maxk.maxk_dense_forward(xe, k, 0.5, seed)[1] * g).sum().backward()
    assert torch.equal(bits(xe.grad), bits(mk.maxk_backward(g, si, d, dropout=(0.5, seed))))
    seen = []

    def backend(gm, example_inputs):
        seen.extend(str(node.target) for node in gm.graph.nodes if node.op == "call_function")
        return gm.forward

    xc = x0.clone().requires_grad_(True)
    torch.compile(step, backend=backend, fullgraph=True)(xc).backward()
    assert sum("maxk_dense_forward" in t for t in seen) == 1, seen
    assert torch.equal(bits(xc.grad), bits(gx))
