"""GPU: feature dropout fused into the MaxK top-k and its backward scatter
(maxk_topk_cbsr_dropout, maxk_scatter_backward_dropout), through the C ABI's Python binding,
the autograd functions, the layers and the torch operators.

The mask is the counter-based hash of include/maxk_hip.h; test_dropout_capi.py restates it in
numpy and the kernels are held to that restatement bit for bit: the expected table is the plain
top-k's table (pinned to the oracle by test_gpu_parity) passed through the numpy mask."""
import numpy as np
import pytest
import torch

import maxk_kernels as mk
from maxk_kernels import graphs
from maxk_kernels.layers import (MaxKGCN, MaxKGCNConv, MaxKGIN, MaxKGINConv, MaxKSAGE,
                                 MaxKSAGEConv)
from oracle import oracle
from test_dropout_capi import drop_scale, dropped_table, keep_mask
from test_gpu_parity import assert_close, graph_on
from test_gpu_records import MODES, SENTINEL, chunk_bytes, pack_records, special_rows
from test_layers import close, dense_adj, maxk_dense, small_edges

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF


def bits(t):
    t = t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32).cpu()


def check_dropout(x, k, mode, p, seed=SEED, layout=None, row_offset=0, stats=True, extra=32):
    """One dropout top-k launch against the plain top-k's table passed through the numpy mask:
    values (bit patterns), selectors, count, record bytes and the statistics pair."""
    n = x.shape[0]
    d0, i0, c0 = mk.maxk_forward(x, k, mode=mode, return_index=True, return_count=True)
    want = torch.from_numpy(dropped_table(d0.cpu().numpy(), i0.cpu().numpy(), p, seed,
                                          row_offset)).to(x.device)
    st = torch.full((2,), -1, dtype=torch.int32, device=x.device) if stats else None
    rec = None
    if layout is not None:
        used = chunk_bytes(layout, k)
        rb = (used + 15) // 16 * 16 + extra
        rec = torch.full((n, rb), SENTINEL, dtype=torch.uint8, device=x.device)
    sd, si, cnt = mk.maxk_forward(x, k, mode=mode, return_index=True, return_count=True,
                                  records=None if rec is None else (rec, layout), stats=st,
                                  dropout=(p, seed, row_offset))
    assert torch.equal(bits(sd), bits(want)), (k, mode, p, layout)
    assert torch.equal(si, i0) and torch.equal(cnt, c0)
    if rec is not None:
        exp = pack_records(want, i0, layout, rb)
        assert torch.equal(rec[:, :used], exp[:, :used]), (k, mode, layout)
        assert bool((rec[:, used:] == SENTINEL).all()), "bytes past the record were written"
    if stats:
        assert st.tolist() == mk.cbsr_stats(want, i0).view(-1).tolist()
    return sd, si, want, d0


# N = 67: no multiple of the rows per wave (4) or per work-group (16); D = 256: the full-row
# kernels; 128: the k > 64 kernels; None: no records, the two plain tables alone
CASES_67 = [(4, 16), (4, 22), (4, 128), (2, 7), (2, 24), (1, 32), (None, 16), (None, 128)]


@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("mode", MODES)
def test_topk_dropout_bit_exact(gpu, mode, p):
    for layout, k in CASES_67:
        x = graphs.features(67, 256, seed=100 + k).to(gpu)
        sd, _, want, d0 = check_dropout(x, k, mode, p, layout=layout)
        check_dropout(x, k, mode, p, layout=layout, stats=False)
    kept = bits(want) != 0
    assert 0.3 < float(kept.float().mean()) < 0.9     # something dropped, something kept


@pytest.mark.parametrize("mode", MODES)
def test_topk_dropout_partial_rows(gpu, mode):
    """D = 100 (partial-row masks) and D = 99 (scalar loads) at n = 5."""
    for d, k in ((100, 8), (99, 10)):
        x = graphs.features(5, d, seed=35 + d).to(gpu)
        for layout in (None, 2, 4):
            check_dropout(x, k, mode, 0.5, layout=layout)


@pytest.mark.parametrize("layout,k", [(4, 16), (2, 7), (4, 66)])
@pytest.mark.parametrize("mode", MODES)
def test_topk_dropout_special_rows(gpu, layout, k, mode):
    """NaN, Inf and denormal inputs: a dropped slot is +0.0f exactly, whatever it held."""
    x = special_rows(256, seed=k).to(gpu)
    sd, si, want, d0 = check_dropout(x, k, mode, 0.5, layout=layout)
    keep = torch.from_numpy(keep_mask(0.5, SEED, np.arange(12)[:, None], si.cpu().numpy()))
    assert bool((bits(sd)[~keep] == 0).all())
    if mode == "exact":     # NaN / Inf entries were selected, some dropped and some kept
        odd = ~torch.isfinite(d0.cpu())
        assert bool((odd & ~keep).any()) and bool((odd & keep).any())


@pytest.mark.parametrize("mode", MODES)
def test_topk_dropout_p0_and_p1(gpu, mode):
    x = graphs.features(67, 256, seed=8).to(gpu)
    for layout, k in ((4, 16), (None, 16), (2, 7)):
        used = chunk_bytes(layout, k) if layout else 0
        outs = []
        for drop in (None, (0.0, SEED)):
            rec = torch.full((67, used + 16), SENTINEL, dtype=torch.uint8, device=gpu)
            st = torch.full((2,), -1, dtype=torch.int32, device=gpu)
            sd, si, cnt = mk.maxk_forward(x, k, mode=mode, return_index=True, return_count=True,
                                          records=(rec, layout) if layout else None, stats=st,
                                          dropout=drop)
            outs.append((bits(sd), si, cnt, rec, st))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        sd, si, cnt = mk.maxk_forward(x, k, mode=mode, return_index=True, return_count=True,
                                      dropout=(1.0, SEED))
        assert bool((bits(sd) == 0).all())
        assert torch.equal(si, outs[0][1]) and torch.equal(cnt, outs[0][2])


@pytest.mark.parametrize("mode", MODES)
def test_topk_dropout_row_offset(gpu, mode):
    """Rows [20, 50) of a 67-row input called with row_offset = 20 equal rows 20..49 of the
    full call: a row's mask does not depend on which call (rank) computes it."""
    x = graphs.features(67, 256, seed=9).to(gpu)
    full, fi = mk.maxk_forward(x, 16, mode=mode, return_index=True, dropout=(0.5, SEED))
    part, pi = mk.maxk_forward(x[20:50].contiguous(), 16, mode=mode, return_index=True,
                               dropout=(0.5, SEED, 20))
    assert torch.equal(bits(part), bits(full[20:50])) and torch.equal(pi, fi[20:50])
    check_dropout(x[20:50].contiguous(), 16, mode, 0.5, layout=4, row_offset=20)
    # past 2^32: the low word of the global row is what counts
    hi, _ = mk.maxk_forward(x[20:50].contiguous(), 16, mode=mode, return_index=True,
                            dropout=(0.5, SEED, 20 + 2 ** 32))
    assert torch.equal(bits(hi), bits(part))


# ------------------------------------------------------------------ scatter
@pytest.mark.parametrize("d,k", [(256, 16), (256, 128), (100, 16)])
def test_scatter_dropout_bit_exact(gpu, d, k):
    n, p = 67, 0.5
    x = graphs.features(n, d, seed=11 + k)
    _, oi = oracle.maxk(x.numpy(), k)
    g = graphs.features(n, k, seed=12 + k)
    want = oracle.maxk_backward(dropped_table(g.numpy(), oi, p, SEED), oi, d)
    got = mk.maxk_backward(g.to(gpu), torch.from_numpy(oi).to(gpu), dim_origin=d,
                           dropout=(p, SEED))
    assert torch.equal(bits(got), bits(want))
    # row offset, p == 0 (the plain kernel) and p == 1
    want = oracle.maxk_backward(dropped_table(g.numpy(), oi, 0.25, 3, 1000), oi, d)
    got = mk.maxk_backward(g.to(gpu), torch.from_numpy(oi).to(gpu), dim_origin=d,
                           dropout=(0.25, 3, 1000))
    assert torch.equal(bits(got), bits(want))
    plain = mk.maxk_backward(g.to(gpu), torch.from_numpy(oi).to(gpu), dim_origin=d)
    got = mk.maxk_backward(g.to(gpu), torch.from_numpy(oi).to(gpu), dim_origin=d,
                           dropout=(0.0, SEED))
    assert torch.equal(bits(got), bits(plain))
    got = mk.maxk_backward(g.to(gpu), torch.from_numpy(oi).to(gpu), dim_origin=d,
                           dropout=(1.0, SEED))
    assert bool((bits(got) == 0).all())
    if k % 4 == 0 and 5 * k <= 128:
        # row-strided u8 selectors: the selector view of layout-1 records
        rec = torch.full((n, 128), SENTINEL, dtype=torch.uint8, device=gpu)
        rec[:, 4 * k:5 * k] = torch.from_numpy(oi).to(gpu)
        sel = rec[:, 4 * k:5 * k]
        assert sel.stride(0) == 128 and not sel.is_contiguous()
        want = oracle.maxk_backward(dropped_table(g.numpy(), oi, p, SEED), oi, d)
        got = mk.maxk_backward(g.to(gpu), sel, dim_origin=d, dropout=(p, SEED))
        assert torch.equal(bits(got), bits(want))


def test_scatter_dropout_repeated_selectors(gpu):
    """The last slot still wins on a repeated selector, with that feature's mask."""
    n, d, k, p = 9, 64, 8, 0.5
    rng = np.random.default_rng(4)
    oi = rng.integers(0, 6, size=(n, k)).astype(np.uint8)      # many repeats
    g = graphs.features(n, k, seed=2)
    want = oracle.maxk_backward(dropped_table(g.numpy(), oi, p, SEED), oi, d)
    got = mk.maxk_backward(g.to(gpu), torch.from_numpy(oi).to(gpu), dim_origin=d,
                           dropout=(p, SEED))
    assert torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------ end to end
N_E2E, E_E2E, D_E2E, P_E2E = 600, 20000, 256, 0.5


@pytest.fixture(scope="module")
def e2e_graph():
    pt, it = graphs.synthetic_csr(N_E2E, E_E2E, seed=41)
    return pt.numpy(), it.numpy(), graphs.sage_mean_values(pt).numpy()


@pytest.mark.parametrize("k", [8, 16, 32])
@pytest.mark.parametrize("mode", MODES)
def test_maxk_aggregate_dropout_end_to_end(gpu, e2e_graph, k, mode):
    """maxk_aggregate(dropout_p) and maxk(dropout_p) + spgemm against the oracle SpGEMM on the
    numpy-dropped oracle table, and x.grad against oracle SSpMM -> mask * scale -> scatter."""
    p, ix, v = e2e_graph
    n, d = N_E2E, D_E2E
    x = graphs.features(n, d, seed=31 + k)
    x[::7, 5] = 1e6                          # ref_compat: single-hit rows with padding slots
    g = graphs.features(n, d, seed=32 + k)
    graph = mk.CSRGraph(*graph_on(gpu, p, ix, v))
    layout = graph.plan(d, k).info()["fwd_layout"]
    if k == 16:
        assert layout == 4
    if k == 8:
        assert layout == 2

    od, oi = oracle.maxk(x.numpy(), k, mode)
    odd = dropped_table(od, oi, P_E2E, SEED)
    ref, mag = oracle.spgemm_forward(p, ix, v, odd, oi, d, with_mag=True)
    gs, gmag = oracle.sspmm_backward(p, ix, v, g.numpy(), oi, with_mag=True)
    scale = float(drop_scale(P_E2E))
    keep = keep_mask(P_E2E, SEED, np.arange(n)[:, None], oi)
    filled = od != 0 if mode == "ref_compat" else np.ones_like(od, bool)
    rows = np.repeat(np.arange(n)[:, None], k, 1)
    gx_ref = np.zeros((n, d))
    gx_mag = np.zeros((n, d))
    gx_ref[rows[filled], oi[filled]] = (gs.astype(np.float64) * keep * scale)[filled]
    gx_mag[rows[filled], oi[filled]] = (gmag.astype(np.float64) * scale)[filled]

    x1 = x.to(gpu).requires_grad_(True)
    y1 = mk.maxk_aggregate(x1, graph, k, mode, dropout_p=P_E2E, seed=SEED)
    y1.backward(g.to(gpu))
    x2 = x.to(gpu).requires_grad_(True)
    sd, si = mk.maxk(x2, k, mode, dropout_p=P_E2E, seed=SEED)
    assert torch.equal(bits(sd), bits(odd))
    y2 = mk.spgemm(sd, si, graph, d)
    y2.backward(g.to(gpu))
    for y, xg in ((y1, x1), (y2, x2)):
        assert_close(y, ref, mag)
        assert_close(xg.grad, gx_ref, gx_mag)
    # not training: today's call
    y3 = mk.maxk_aggregate(x.to(gpu), graph, k, mode, dropout_p=P_E2E, training=False)
    assert torch.equal(y3, mk.maxk_aggregate(x.to(gpu), graph, k, mode))


def test_dropout_seed_comes_from_the_torch_generator(gpu, e2e_graph):
    p, ix, v = e2e_graph
    graph = mk.CSRGraph(*graph_on(gpu, p, ix, v))
    x = graphs.features(N_E2E, D_E2E, seed=3).to(gpu)

    def run(seed):
        torch.manual_seed(seed)
        sd, si = mk.maxk(x, 16, dropout_p=0.5)
        torch.manual_seed(seed)
        return sd, mk.maxk_aggregate(x, graph, 16, dropout_p=0.5)

    (a, ya), (b, yb), (c, yc) = run(5), run(5), run(6)
    assert torch.equal(bits(a), bits(b)) and not torch.equal(bits(a), bits(c))
    assert torch.allclose(ya, yb, rtol=1e-5, atol=1e-6) and not torch.allclose(ya, yc, rtol=1e-3)
    torch.manual_seed(5)
    drawn = torch.empty((), dtype=torch.int64).random_().item()
    sd, _ = mk.maxk(x, 16, dropout_p=0.5, seed=drawn)
    assert torch.equal(bits(sd), bits(a))
    with pytest.raises(ValueError):
        mk.maxk(x, 16, dropout_p=1.5)


# ------------------------------------------------------------------ layers
def _drawn_seed(s):
    """The seed a layer's one fused-dropout call draws right after torch.manual_seed(s)."""
    torch.manual_seed(s)
    seed = torch.empty((), dtype=torch.int64).random_().item()
    torch.manual_seed(s)
    return seed


def _mask64(p, seed, n, d):
    """The [n, d] dropout factor keep * scale as float64."""
    keep = keep_mask(p, seed, np.arange(n)[:, None], np.arange(d)[None, :])
    return torch.from_numpy(keep.astype(np.float64) * float(drop_scale(p)))


@pytest.mark.parametrize("kind", ["sage", "sage_after_fc", "gcn", "gin"])
def test_layers_fused_dropout_match_dense(gpu, kind):
    dst, src, n = small_edges()
    csr = mk.CSRGraph.from_edges(src.to(gpu), dst.to(gpu), n)
    k, p, d = 16, 0.5, 64
    torch.manual_seed(0)
    make = {
        "sage": lambda fd: MaxKSAGEConv(d, 48, "mean", feat_drop=p, maxk=k, fused_dropout=fd),
        "sage_after_fc": lambda fd: MaxKSAGEConv(d, d, "mean", feat_drop=p, maxk=k, bias=False,
                                                 maxk_after_fc=True, fused_dropout=fd),
        "gcn": lambda fd: MaxKGCNConv(d, d, norm="both", feat_drop=p, maxk=k, fused_dropout=fd,
                                      allow_zero_in_degree=True),
        "gin": lambda fd: MaxKGINConv(d, maxk=k, feat_drop=p, fused_dropout=fd),
    }[kind]
    conv = make(True).to(gpu)
    plain = make(False).to(gpu)
    plain.load_state_dict(conv.state_dict())
    x = graphs.features(n, d, seed=3).to(gpu).requires_grad_(True)
    w = graphs.features(n, 48 if kind == "sage" else d, seed=4).to(gpu)
    seed = _drawn_seed(17)
    y = conv.train()(csr, x)
    (y * w).sum().backward()

    M = _mask64(p, seed, n, d)
    xr = x.detach().cpu().double().requires_grad_(True)
    P = {name: t.detach().cpu().double() for name, t in conv.named_parameters()}
    if kind == "sage":
        xm = maxk_dense(xr, k) * M
        yr = xm @ P["fc_self.weight"].T + (dense_adj(csr, "mean") @ xm) @ P["fc_neigh.weight"].T \
            + P["bias"]
    elif kind == "sage_after_fc":
        yr = xr @ P["fc_self.weight"].T + dense_adj(csr, "mean") @ (
            maxk_dense(xr @ P["fc_neigh.weight"].T, k) * M)
    elif kind == "gcn":
        yr = dense_adj(csr, "both") @ (maxk_dense(xr @ P["weight"], k) * M) + P["bias"]
    else:
        xm = maxk_dense(xr, k) * M
        yr = (1 + P["eps"]) * xm + dense_adj(csr, "sum") @ xm
    (yr * w.cpu().double()).sum().backward()
    assert close(y, yr), float((y.detach().double().cpu() - yr).abs().max())
    assert close(x.grad, xr.grad)
    # eval mode does not depend on the switch
    with torch.no_grad():
        assert torch.equal(conv.eval()(csr, x), plain.eval()(csr, x))


@pytest.mark.parametrize("model_cls", [MaxKSAGE, MaxKGCN, MaxKGIN])
def test_model_trains_with_fused_dropout(gpu, model_cls):
    """test_layers.test_model_trains with fused_dropout=True (same graph, sizes, feat_drop)."""
    dst, src, n = small_edges(n=800, e=16000, seed=11)
    csr = mk.CSRGraph.from_edges(src.to(gpu), dst.to(gpu), n)
    torch.manual_seed(3)
    feats = graphs.features(n, 32, seed=12).to(gpu)
    labels = torch.randint(0, 5, (n,), generator=torch.Generator().manual_seed(1)).to(gpu)
    model = model_cls(32, 64, 2, 5, maxk=16, feat_drop=0.1, norm=True, fused_dropout=True).to(gpu)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(csr, feats), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0] - 0.1


# ------------------------------------------------------------------ torch operators
def test_torch_ops_dropout(gpu):
    n, d, k, p = 300, 64, 16, 0.5
    seed = -1234567890123456789                      # int64 schema int, read as uint64
    x0 = graphs.features(n, d, seed=1).to(gpu)
    sd, si = torch.ops.maxk.maxk_dropout_forward(x0, k, p, seed)
    ed, ei = mk.maxk_forward(x0, k, return_index=True, dropout=(p, seed % 2 ** 64))
    assert torch.equal(bits(sd), bits(ed)) and torch.equal(si, ei)
    assert bool((bits(sd) == 0).any())
    g = graphs.features(n, k, seed=2).to(gpu)
    gx = torch.ops.maxk.maxk_dropout_backward(g, si, d, p, seed)
    assert torch.equal(bits(gx), bits(mk.maxk_backward(g, si, d, dropout=(p, seed))))
    torch.library.opcheck(torch.ops.maxk.maxk_dropout_forward.default, (x0, k, p, seed))
    torch.library.opcheck(torch.ops.maxk.maxk_dropout_backward.default, (g, si, d, p, seed))

    def step(x):
        data, _ = torch.ops.maxk.maxk_dropout_forward(x, k, p, seed)
        return (data * g).sum()

    xe = x0.clone().requires_grad_(True)
    step(xe).backward()
    assert torch.equal(bits(xe.grad), bits(gx))      # the registered derivative
    seen = []

    def backend(gm, example_inputs):
        seen.extend(str(node.target) for node in gm.graph.nodes if node.op == "call_function")
        return gm.forward

    xc = x0.clone().requires_grad_(True)
    torch.compile(step, backend=backend, fullgraph=True)(xc).backward()
    assert sum("maxk_dropout_forward" in t for t in seen) == 1, seen
    assert torch.equal(bits(xc.grad), bits(gx))
