"""GPU: the top-k writes the forward's chunk records (maxk_topk_cbsr_records) and the forward
gathers them as they are (maxk_spgemm_forward_records), through the C ABI, the Python package
and maxk_aggregate.

The expected record bytes are packed here in torch from the tables the plain top-k returns
(pinned bit-exact to the oracle by test_gpu_parity), by the layout table of maxk_hip.h."""
import ctypes

import numpy as np
import pytest
import torch

import maxk_kernels as mk
from maxk_kernels import _lib, graphs
from oracle import oracle
from test_gpu_parity import _stat_rows, assert_close, graph_on

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
MODES = ["exact", "ref_compat"]


def chunk_bytes(layout, k):
    """Bytes of a row's record that the top-k writes."""
    return {1: 5 * k, 2: 16 * ((k + 2) // 3), 4: 16 * (k // 2)}[layout]


def pack_records(sd, si, layout, rb):
    """[n, rb] u8 records of the plain tables sd f32 [n, k], si u8 [n, k]; bytes past the
    record's chunks hold SENTINEL."""
    n, k = sd.shape
    rec = torch.full((n, rb), SENTINEL, dtype=torch.uint8, device=sd.device)
    bits = sd.contiguous().view(torch.int32)        # bit patterns (NaN payloads survive)
    if layout == 1:
        rec[:, :4 * k] = bits.view(torch.uint8).view(n, 4 * k)
        rec[:, 4 * k:5 * k] = si
        return rec
    v = 3 if layout == 2 else 2
    chunks = (k + v - 1) // v
    xb = torch.zeros((n, chunks * v), dtype=torch.int32, device=sd.device)
    xb[:, :k] = bits
    sb = torch.zeros((n, chunks * v), dtype=torch.int32, device=sd.device)
    sb[:, :k] = si.to(torch.int32)
    xb, sb = xb.view(n, chunks, v), sb.view(n, chunks, v)
    words = torch.zeros((n, chunks, 4), dtype=torch.int32, device=sd.device)
    words[:, :, :v] = xb
    sel = torch.zeros((n, chunks), dtype=torch.int32, device=sd.device)
    for i in range(v):
        sel |= sb[:, :, i] << (8 * i)
    words[:, :, 3 if v == 3 else 2] = sel
    rec[:, :16 * chunks] = words.view(n, chunks * 4).view(torch.uint8).view(n, 16 * chunks)
    return rec


def check_records(x, k, mode, layout, stats=False, extra=32):
    """One maxk_topk_cbsr_records launch against the plain top-k of the same input."""
    n = x.shape[0]
    d0, i0, c0 = mk.maxk_forward(x, k, mode=mode, return_index=True, return_count=True)
    used = chunk_bytes(layout, k)
    rb = (used + 15) // 16 * 16 + extra
    rec = torch.full((n, rb), SENTINEL, dtype=torch.uint8, device=x.device)
    st = torch.full((2,), -1, dtype=torch.int32, device=x.device) if stats else None
    sd, si, cnt = mk.maxk_forward(x, k, mode=mode, return_index=True, return_count=True,
                                  records=(rec, layout), stats=st)
    want = pack_records(d0, i0, layout, rb)
    assert torch.equal(rec[:, :used], want[:, :used]), (k, mode, layout)
    assert bool((rec[:, used:] == SENTINEL).all()), "bytes past the record were written"
    assert torch.equal(si, i0)
    assert torch.equal(sd.view(torch.int32), d0.view(torch.int32))
    assert torch.equal(cnt, c0)
    if stats:
        assert st.tolist() == mk.cbsr_stats(d0, i0).view(-1).tolist()
    return rec, d0, i0


# N = 67: no multiple of the rows per wave (4) or per work-group (16); D = 256: the full-row
# kernels. 22: k % 4 == 2; 7: last lane chunk partly padding; 128 / 192: 64 chunks, k > 64 kernels
CASES_67 = ([(4, k) for k in (2, 16, 22, 64, 128)] + [(2, k) for k in (1, 7, 8, 24, 192)] +
            [(1, k) for k in (8, 16)])


@pytest.mark.parametrize("layout,k", CASES_67)
@pytest.mark.parametrize("mode", MODES)
def test_record_bytes_bit_exact(gpu, layout, k, mode):
    x = graphs.features(67, 256, seed=100 + k).to(gpu)
    check_records(x, k, mode, layout)


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("mode", MODES)
def test_record_bytes_partial_rows(gpu, n, mode):
    """D = 100 (partial-row masks, D % 4 == 0) and D = 99 (scalar loads), and D = k = 16 (every
    feature selected), in every layout."""
    for d, k in ((100, 6), (100, 8), (99, 10), (16, 16)):
        x = graphs.features(n, d, seed=7 * n + d).to(gpu)
        for layout in (1, 2, 4):
            if layout == 1 and k % 4:
                continue
            check_records(x, k, mode, layout)
            check_records(x, k, mode, layout, stats=True)


def special_rows(d, seed):
    """Random rows, then: all values equal, NaNs of both signs with +-Inf, denormals, zeros, a
    single spike (ref_compat fills fewer than k slots on several of them)."""
    x = graphs.features(12, d, seed=seed)
    x[3] = 0.75
    x[4, 7] = float("nan")
    x[4, 9] = float("inf")
    x[4, 11] = -float("inf")
    x[4, 200] = torch.from_numpy(np.array([0xffc00001], np.uint32).view(np.float32))[0]
    x[5] = torch.from_numpy(np.array([0xffc00000] * d, np.uint32).view(np.float32))
    x[6] = 1e-40
    x[6, 3] = -1e-41
    x[7] = 0.0
    x[8] = 0.0
    x[8, 100] = 1e6
    return x


@pytest.mark.parametrize("layout,k", [(2, 7), (2, 8), (4, 16), (4, 6), (1, 16), (2, 70), (4, 66)])
@pytest.mark.parametrize("mode", MODES)
def test_record_bytes_special_rows(gpu, layout, k, mode):
    x = special_rows(256, seed=k).to(gpu)
    check_records(x, k, mode, layout)
    check_records(x, k, mode, layout, stats=True)


def test_record_bytes_large_input(gpu):
    """N past the row count where the plain exact kernel takes 8 rows per wave (2^20), not a
    multiple of anything; 64 MB of input. No statistics."""
    n, d, k = (1 << 20) + 3, 16, 8
    gen = torch.Generator(device=gpu).manual_seed(5)
    x = torch.randn((n, d), device=gpu, generator=gen)
    rec, _, _ = check_records(x, k, "exact", 2)
    assert rec.shape == (n, 80)


def test_records_without_plain_tables(gpu):
    """sp_data and sp_index NULL: only the records (and the count) are written, through the C
    entry point; return_values=False through the package."""
    n, d, k = 67, 256, 16
    x = graphs.features(n, d, seed=3).to(gpu)
    d0, i0 = mk.maxk_forward(x, k, mode="ref_compat", return_index=True)
    want = pack_records(d0, i0, 4, 128)
    rec = torch.full((n, 128), SENTINEL, dtype=torch.uint8, device=gpu)
    P = ctypes.c_void_p
    stream = P(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib.maxk_topk_cbsr_records(P(x.data_ptr()), P(rec.data_ptr()), 128, 4, None, 0,
                                         None, 0, None, None, None, 0, n, d, k, 1, stream)
    assert rc == 0, _lib.lib.maxk_last_error()
    assert torch.equal(rec, want)
    rec.fill_(SENTINEL)
    res = mk.maxk_forward(x, k, mode="ref_compat", return_index=True, records=(rec, 4),
                          return_values=False)
    assert res[0] is None and torch.equal(res[1], i0) and torch.equal(rec, want)
    with pytest.raises(RuntimeError, match="return_values"):
        mk.maxk_forward(x, k, return_values=False)


@pytest.mark.parametrize("layout,k", [(2, 8), (2, 24), (4, 16), (4, 24), (2, 1), (4, 64)])
@pytest.mark.parametrize("mode", MODES)
def test_records_fused_stats_equal_cbsr_stats(gpu, layout, k, mode):
    """The pair written with the records equals maxk_cbsr_stats of the plain tables bit for
    bit, on random rows and with each special row of test_topk_fused_stats_equal_cbsr_stats
    in turn setting the pair."""
    n, d = 1000, 256
    base = graphs.features(n, d, seed=k)
    special = _stat_rows(16, d, seed=k + 1)
    for r in [None] + list(range(3, 10)):
        x = base.clone()
        if r is not None:
            x[777] = special[r]
        check_records(x.to(gpu), k, mode, layout, stats=True)


# ------------------------------------------------------------------ forward from records
N_FWD, E_FWD, D_FWD = 2000, 300_000, 256


@pytest.fixture(scope="module")
def fwd_graph():
    pt, it = graphs.synthetic_csr(N_FWD, E_FWD, seed=37)
    return pt.numpy(), it.numpy(), graphs.sage_mean_values(pt).numpy()


@pytest.fixture(scope="module")
def fwd_refs(fwd_graph):
    """Per k: input, oracle tables and oracle forward (computed once, shared, never changed)."""
    p, ix, v = fwd_graph
    refs = {}

    def get(k):
        if k not in refs:
            x = graphs.features(N_FWD, D_FWD, seed=50 + k)
            od, oi = oracle.maxk(x.numpy(), k)
            ref, mag = oracle.spgemm_forward(p, ix, v, od, oi, D_FWD, with_mag=True)
            refs[k] = (x, ref, mag)
        return refs[k]
    return get


def run_forward_records(gpu, plan, x, layout_expected):
    """top-k -> records (+ statistics when the plan is fixed point) -> forward_records; also
    the plain tables and the pair."""
    info = plan.info()
    assert info["fwd_layout"] == layout_expected
    rec, layout = plan.new_records()
    assert layout == layout_expected and rec.shape == (plan.num_cols, info["fwd_record_bytes"])
    st = torch.empty(2, dtype=torch.int32, device=gpu)
    sd, si = mk.maxk_forward(x, plan.dim_k, return_index=True, records=(rec, layout), stats=st)
    y = plan.forward_records(rec, layout, stats=st.view(1, 2))
    return y, rec, layout, sd, si, st


@pytest.mark.parametrize("k,options,layout", [
    (8, {}, 2), (16, {}, 4), (24, {}, 2), (16, {"fwd_chunk3": 2}, 1),
    (16, {"fwd_task_cap": 150}, 4), (8, {"fwd_task_cap": 150}, 2),
])
def test_forward_from_records(gpu, fwd_graph, fwd_refs, k, options, layout):
    p, ix, v = fwd_graph
    x, ref, mag = fwd_refs(k)
    ptr, idx, val = graph_on(gpu, p, ix, v)
    plan = mk.GraphPlan(ptr, idx, val, N_FWD, ix.size, D_FWD, k, options=options)
    info = plan.info()
    # rows longer than the cap are split into segments whose partial sums meet in f32 global
    # atomics: their order, and so the row's last bit, varies from launch to launch (of
    # plan.forward too), so those rows are held to the oracle bound only
    whole = torch.ones(N_FWD, dtype=torch.bool)
    if "fwd_task_cap" in options:
        whole = torch.from_numpy(np.diff(p) <= options["fwd_task_cap"])
        assert info["fwd_split_rows"] == int((~whole).sum()) and 0 < int(whole.sum()) < N_FWD
    else:
        assert info["fwd_split_rows"] == 0
    whole = whole.to(gpu)
    assert info["fwd_fixed"] == (1 if k >= 16 else 0)
    y, rec, lay, sd, si, st = run_forward_records(gpu, plan, x.to(gpu), layout)
    assert_close(y, ref, mag)
    if info["fwd_fixed"] == 1:   # integer sums, the same statistics
        assert torch.equal(y[whole], plan.forward(sd, si, stats=st.view(1, 2))[whole])
    # a second call into the same (dirty) output: split rows are zeroed again
    y2 = plan.forward_records(rec, lay, out=y.clone().fill_(3.0), stats=st.view(1, 2))
    assert_close(y2, ref, mag)
    # accumulate into a prefilled output
    pre = graphs.features(N_FWD, D_FWD, seed=9)
    out = pre.clone().to(gpu)
    plan.forward_records(rec, lay, out=out, accumulate=True, stats=st.view(1, 2))
    assert_close(out, ref + pre.numpy().astype(np.float64), mag + np.abs(pre.numpy()))
    with pytest.raises(RuntimeError, match="accumulate"):
        plan.forward_records(rec, lay, accumulate=True)
    # a record stride other than the plan's own
    wide = torch.empty((plan.num_cols, rec.shape[1] + 48), dtype=torch.uint8, device=gpu)
    wide[:, :rec.shape[1]] = rec
    yw = plan.forward_records(wide, lay, stats=st.view(1, 2))
    assert_close(yw, ref, mag)
    if info["fwd_fixed"] == 1:
        assert torch.equal(yw[whole], y[whole])


@pytest.mark.parametrize("num_cols,k,layout", [(1, 16, 4), (5, 8, 2), (5, 16, 4), (1, 8, 2)])
def test_forward_from_records_rectangular(gpu, num_cols, k, layout):
    rng = np.random.default_rng(num_cols)
    n, d = 300, 256
    rows = [np.sort(rng.choice(num_cols, size=rng.integers(0, num_cols + 1), replace=False))
            for _ in range(n)]
    p = np.zeros(n + 1, np.int32)
    p[1:] = np.cumsum([len(r) for r in rows])
    ix = np.concatenate(rows).astype(np.int32)
    v = rng.standard_normal(ix.size).astype(np.float32)
    x = graphs.features(num_cols, d, seed=num_cols + k)
    od, oi = oracle.maxk(x.numpy(), k)
    # the oracle is square: tables padded to n rows (no edge points at the padding)
    odp, oip = np.zeros((n, k), np.float32), np.zeros((n, k), np.uint8)
    odp[:num_cols], oip[:num_cols] = od, oi
    ref, mag = oracle.spgemm_forward(p, ix, v, odp, oip, d, with_mag=True)
    ptr, idx, val = graph_on(gpu, p, ix, v)
    plan = mk.GraphPlan(ptr, idx, val, n, ix.size, d, k, num_cols=num_cols)
    y, *_ = run_forward_records(gpu, plan, x.to(gpu), layout)
    assert_close(y, ref, mag)


def test_forward_records_c_entry_point_and_refusals(gpu, fwd_graph, fwd_refs):
    """The C entry point on the external-workspace plan GraphPlan builds: it has no workspace
    parameter, so nothing is packed into scratch. Refusals: another layout than the plan's, a
    fixed-point plan without statistics, a plan that gathers the plain tables."""
    p, ix, v = fwd_graph
    k = 16
    x, ref, mag = fwd_refs(k)
    ptr, idx, val = graph_on(gpu, p, ix, v)
    plan = mk.GraphPlan(ptr, idx, val, N_FWD, ix.size, D_FWD, k)
    assert plan.external and plan.fwd_ws_bytes > 0 and plan.info()["fwd_fixed"] == 1
    rec, layout = plan.new_records()
    st = torch.empty(2, dtype=torch.int32, device=gpu)
    mk.maxk_forward(x.to(gpu), k, return_index=True, records=(rec, layout), stats=st,
                    return_values=False)
    out = torch.empty((N_FWD, D_FWD), device=gpu)
    P = ctypes.c_void_p
    lib = _lib.lib

    def call(lay, stats):
        return lib.maxk_spgemm_forward_records(
            plan.handle, P(ptr.data_ptr()), P(idx.data_ptr()), P(val.data_ptr()),
            P(rec.data_ptr()), rec.shape[1], lay, P(out.data_ptr()), N_FWD, ix.size, k, D_FWD, 0,
            P(stats.data_ptr()) if stats is not None else None, 1 if stats is not None else 0, 0,
            P(torch.cuda.current_stream().cuda_stream))

    assert call(layout, st) == 0, lib.maxk_last_error()
    assert_close(out, ref, mag)
    assert call(2, st) == -3 and b"maxk_spgemm_forward_records" in lib.maxk_last_error()
    assert call(1, st) == -3
    assert call(layout, None) == -1 and b"stats" in lib.maxk_last_error()
    with pytest.raises(_lib.MaxKError, match="code -3"):
        plan.forward_records(rec, 2, stats=st.view(1, 2))
    with pytest.raises(_lib.MaxKError, match="code -1"):
        plan.forward_records(rec, layout)
    # k = 32 gathers the two plain tables here: nothing to hand in
    plan32 = mk.GraphPlan(ptr, idx, val, N_FWD, ix.size, D_FWD, 32)
    assert plan32.info()["fwd_layout"] == 0 and plan32.new_records() is None
    rec32 = torch.zeros((N_FWD, 256), dtype=torch.uint8, device=gpu)
    with pytest.raises(_lib.MaxKError, match="code -2"):
        plan32.forward_records(rec32, 4, stats=st.view(1, 2))
    # new_cbsr keeps its behaviour: plain tables at layouts 2 and 4, record views at layout 1
    sd, si = plan.new_cbsr()
    assert sd.is_contiguous() and si.is_contiguous() and sd.shape == (N_FWD, k)
    plan1 = mk.GraphPlan(ptr, idx, val, N_FWD, ix.size, D_FWD, k, options={"fwd_chunk3": 2})
    sd, si = plan1.new_cbsr()
    assert si.stride(0) == plan1.info()["fwd_record_bytes"] == 128


# ------------------------------------------------------------------ maxk_aggregate
class _GraphWithPlan(mk.CSRGraph):
    """A graph that hands out one plan built with options (the cache builds default plans)."""
    fixed_plan = None

    def plan(self, dim_origin, dim_k):
        assert (self.fixed_plan.dim_origin, self.fixed_plan.dim_k) == (dim_origin, dim_k)
        return self.fixed_plan


@pytest.mark.parametrize("k,options,layout", [(8, None, 2), (16, None, 4), (24, None, 2),
                                              (16, {"fwd_chunk3": 2}, 1)])
@pytest.mark.parametrize("mode", MODES)
def test_maxk_aggregate_from_records(gpu, fwd_graph, k, options, layout, mode):
    """test_maxk_aggregate_fused_equals_unfused for the record path: maxk_aggregate (top-k
    writing the plan's records, forward gathering them, no pack or statistics pass) against
    MaxKFunction -> SpGEMMFunction and the oracle, at the default layouts and on a packed
    (layout 1) plan; bitwise equal outputs where the forward is fixed point."""
    p, ix, v = fwd_graph
    n, d = N_FWD, D_FWD
    x = graphs.features(n, d, seed=31 + k)
    x[::7, 5] = 1e6                          # ref_compat: single-hit rows with padding slots
    g = graphs.features(n, d, seed=32 + k).to(gpu)
    graph = mk.CSRGraph(*graph_on(gpu, p, ix, v))
    if options is not None:                  # the plan both compositions get from the graph
        graph = _GraphWithPlan(graph.ptr, graph.idx, graph.val)
        graph.fixed_plan = mk.GraphPlan(graph.ptr, graph.idx, graph.val, n, ix.size, d, k,
                                        options=options)
    plan = graph.plan(d, k)
    assert plan.info()["fwd_layout"] == layout and plan.new_records() is not None
    x1 = x.to(gpu).requires_grad_(True)
    y1 = mk.maxk_aggregate(x1, graph, k, mode)
    y1.backward(g)
    x2 = x.to(gpu).requires_grad_(True)
    sd, si = mk.maxk(x2, k, mode)
    y2 = mk.spgemm(sd, si, graph, d)
    y2.backward(g)
    if plan.info()["fwd_fixed"] == 1:
        assert torch.equal(y1, y2)
    od, oi = oracle.maxk(x.numpy(), k, mode)
    ref, mag = oracle.spgemm_forward(p, ix, v, od, oi, d, with_mag=True)
    assert_close(y1, ref, mag)
    assert_close(y2, ref, mag)
    gs, gmag = oracle.sspmm_backward(p, ix, v, g.cpu().numpy(), oi, with_mag=True)
    filled = od != 0 if mode == "ref_compat" else np.ones_like(od, bool)
    gx_ref = np.zeros((n, d))
    gx_mag = np.zeros((n, d))
    rows = np.repeat(np.arange(n)[:, None], k, 1)
    gx_ref[rows[filled], oi[filled]] = gs[filled]      # ascending unique selectors per row
    gx_mag[rows[filled], oi[filled]] = gmag[filled]
    assert_close(x1.grad, gx_ref, gx_mag)
    assert_close(x2.grad, gx_ref, gx_mag)


def test_maxk_backward_row_strided_u8_indices(gpu):
    """maxk_backward reading u8 selectors at a row stride (rec[:, 4k:5k] of a layout-1 record
    buffer) against the oracle."""
    n, d, k = 203, 256, 16
    x = graphs.features(n, d, seed=11)
    _, oi = oracle.maxk(x.numpy(), k)
    g = graphs.features(n, k, seed=12)
    rec = torch.full((n, 128), SENTINEL, dtype=torch.uint8, device=gpu)
    rec[:, 4 * k:5 * k] = torch.from_numpy(oi).to(gpu)
    sel = rec[:, 4 * k:5 * k]
    assert sel.stride(0) == 128 and not sel.is_contiguous()
    got = mk.maxk_backward(g.to(gpu), sel, dim_origin=d)
    assert np.array_equal(got.cpu().numpy(), oracle.maxk_backward(g.numpy(), oi, d))
