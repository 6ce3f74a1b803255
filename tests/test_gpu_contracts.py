"""GPU: the output contracts of include/maxk_hip.h, through the C ABI, on buffers the test owns.

The parity tests hand every kernel a fresh ``torch.empty`` of exactly the documented size, so
three defects pass them by construction: an output element that is never written (the expected
zero is whatever the allocator returned), a store just past an output or past the reported
scratch size (it lands in the allocator's slack), and a result that depends on what the scratch
held before. Here every output and every scratch buffer is the payload of a poisoned, guarded
arena (tests/arena.py), each case runs once per poison pattern, and after a synchronise every
case checks

  (a) each payload element against the bar the suite uses for that output: bit-exact against
      oracle.maxk / oracle.maxk_backward and the numpy restatements of test_dropout_capi.py /
      test_self_capi.py (top-k, scatter, records, dense, count, statistics), oracle.close_enough
      at RTOL = 1e-5 (forward, backward, dense SpMM); surviving poison passes neither;
  (b) both guards and every stride gap of every arena;
  (c) every input tensor bit for bit against a clone taken before the call.

Two places where the check is stated more exactly than "bit-exact" or "nothing": the dense SpMM is
held to RTOL = 1e-5 of an f64-accumulated reference (the oracle's forward over a table that
selects every feature), a tighter bar than test_dense_spmm_vs_oracle's f32 one; and a top-k over
no rows writes nothing except the statistics pair, which the header defines as all zero
(test_topk_fused_stats_empty_and_tiny relies on it).
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import maxk_kernels as mk
from arena import POISONS, Arena
from maxk_kernels import _lib, graphs
from oracle import oracle
from test_dropout_capi import drop_scale, dropped_table, keep_mask
from test_gpu_parity import GRAPHS, PLAN_OPTIONS, RTOL
from test_gpu_records import chunk_bytes, pack_records
from test_gpu_self import _filled_count
from test_self_capi import dense_rows, merge_rows

pytestmark = pytest.mark.gpu

lib = _lib.lib
P = ctypes.c_void_p
MODES = ["exact", "ref_compat"]
SEED = 0x0123456789ABCDEF
ROW_OFFSET = 3                     # the dropout mask is keyed on row_offset + r
F32, U8, I32 = torch.float32, torch.uint8, torch.int32

# what ran, for test_contract_coverage_report (file order: it runs last)
CASES = {f: 0 for f in ("top-k", "scatter", "forward", "backward", "dense and statistics",
                        "autograd")}
SEEN = {"fwd": set(), "accumulate": set(), "bwd_algo": set(), "autograd_arenas": 0}
T0 = time.time()


def stream():
    return P(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device address of a tensor or an arena's payload; None (NULL) for None."""
    if t is None:
        return None
    return P(t.ptr if isinstance(t, Arena) else t.data_ptr())


def raw(t):
    if t.numel() == 0:
        return torch.empty(0, dtype=torch.uint8, device=t.device)
    return t.contiguous().reshape(-1).view(torch.uint8)


class Call:
    """The buffers of one C call: arenas for what it writes, clones of what it reads."""

    def __init__(self, dev, poison, what):
        self.dev, self.poison, self.what = dev, poison, what
        self.arenas, self.inputs = {}, {}

    def out(self, name, spec):
        self.arenas[name] = a = Arena(spec, self.dev, self.poison)
        return a

    def inp(self, name, t):
        t = (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t)
        t = t.to(self.dev)
        self.inputs[name] = (t, t.clone())
        return t

    def ok(self, rc):
        assert rc == 0, (self.what, rc, lib.maxk_last_error())

    def done(self):
        """(b) and (c), after a synchronise."""
        torch.cuda.synchronize()
        for name, a in self.arenas.items():
            bad = a.check()
            assert bad is None, f"{self.what}: write outside the payload of {name}: {bad}"
        for name, (t, clone) in self.inputs.items():
            assert torch.equal(raw(t), raw(clone)), f"{self.what}: input {name} was modified"

    def untouched(self, name):
        a = self.arenas[name]
        assert bool((a.buf == a.poison).all()), f"{self.what}: {name} was written"


def host(a):
    return a.payload.contiguous().cpu().numpy()


def assert_bits(call, name, want):
    """Payload `name` equals `want` (numpy, same dtype) bit for bit."""
    got = host(call.arenas[name])
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (call.what, name, got.shape)
    w = {4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
    diff = np.argwhere(got.view(w) != want.view(w))
    assert diff.size == 0, (f"{call.what}: {name} differs at {tuple(diff[0])}: got "
                            f"{got.view(w)[tuple(diff[0])]:#x}, want "
                            f"{want.view(w)[tuple(diff[0])]:#x} ({len(diff)} elements)")


def assert_bar(call, got, ref, mag, name):
    ok, worst = oracle.close_enough(got, ref, mag, rtol=RTOL)
    assert ok, f"{call.what}: {name}: worst err/bound {worst:.3g}"


def assert_written(call, name):
    hole = call.arenas[name].first_poisoned()
    assert hole is None, f"{call.what}: {name}{list(hole)} was never written"


# =========================================================================== top-k
TOPK_N = [1, 3, 5, 9, 67]          # no multiple of the rows per wave (4 / 8) or per work-group
TOPK_DK = [(256, 16), (256, 66), (256, 256), (100, 5), (37, 37), (7, 3), (1, 1)]
TOPK_ENTRIES = ["cbsr", "count", "tables", "ex", "records", "dropout", "dense", "dense_p0"]
HAS = {  # outputs each entry point takes
    "cbsr": (), "count": ("count",), "tables": ("count", "strides"),
    "ex": ("count", "strides", "stats"),
    "records": ("count", "strides", "stats", "records"),
    "dropout": ("count", "strides", "stats", "records"),
    "dense": ("count", "strides", "stats", "records", "dense"),
    "dense_p0": ("count", "strides", "stats", "records", "dense"),
}
NULLS = {  # the NULL-able outputs, given as NULL in turn
    "count": [{"count"}], "tables": [{"count"}], "ex": [{"count"}, {"stats"}],
    "records": [{"count"}, {"stats"}, {"sp_data"}, {"sp_index"}, {"sp_data", "sp_index"}],
    "dropout": [{"records"}, {"sp_data"}, {"sp_index"}, {"count", "stats"}],
    "dense": [{"records"}, {"sp_data"}, {"sp_index"}, {"records", "sp_data", "sp_index"},
              {"stats"}, {"count"}],
    "dense_p0": [{"records", "sp_data", "sp_index"}, {"stats", "count"}],
}
_TOPK_REF = {}


def layouts_for(k):
    out = []
    if k % 4 == 0:
        out.append(1)
    if (k + 2) // 3 <= 64:
        out.append(2)
    if k % 2 == 0 and k // 2 <= 64:
        out.append(4)
    return out


def stats_pair(values):
    """maxk_cbsr_stats over rows that never repeat a nonzero selector: the bit patterns of
    max |x| and 0x7fffffff - min nonzero |x| (finite values: bit order is magnitude order)."""
    a = np.abs(np.ascontiguousarray(values, np.float32)).view(np.uint32)
    nz = a[a != 0]
    if nz.size == 0:
        return np.zeros(2, np.int32)
    return np.array([int(a.max()), 0x7FFFFFFF - int(nz.min())], np.uint32).view(np.int32)


def topk_ref(n, d, k, mode, p):
    """Expected outputs of one top-k launch, computed once per shape (never modified)."""
    key = (n, d, k, mode, p)
    if key not in _TOPK_REF:
        x = graphs.features(n, d, seed=1000 + 7 * d + k + n)
        od, oi = oracle.maxk(x.numpy(), k, mode)
        cnt = (np.full(n, k) if mode == "exact" else _filled_count(od, oi)).astype(np.int32)
        val = dropped_table(od, oi, p, SEED, ROW_OFFSET) if p else od
        ref = dict(x=x, values=val, index=oi, count=cnt, stats=stats_pair(val),
                   dense=dense_rows(val, oi, cnt, d), records={})
        tv, ti = torch.from_numpy(val), torch.from_numpy(oi)
        for layout in layouts_for(k):
            used = chunk_bytes(layout, k)
            ref["records"][layout] = pack_records(tv, ti, layout, used)[:, :used].numpy()
        _TOPK_REF[key] = ref
    return _TOPK_REF[key]


def run_topk(gpu, poison, entry, mode, n, d, k, strided, null=frozenset(), layout=None, rows=None):
    """One launch of `entry` on n rows; `rows` > n sizes the arenas for more rows than the call
    is told about (N = 0: nothing may be written)."""
    p = 0.5 if entry in ("dropout", "dense") else 0.0
    has = HAS[entry]
    ref = topk_ref(rows or n, d, k, mode, p)
    what = f"top-k {entry} {mode} N={n} D={d} k={k} strided={strided} null={sorted(null)} " \
           f"layout={layout} poison={poison:#x}"
    c = Call(gpu, poison, what)
    m = rows or n
    x = c.inp("in", ref["x"])
    ds, is_ = (k + 3, k + 1) if strided else (k, k)
    sd = None if "sp_data" in null else c.out("sp_data", (m, k, F32, ds))
    si = None if "sp_index" in null else c.out("sp_index", (m, k, U8, is_))
    cnt = c.out("count", (1, m, I32)) if "count" in has and "count" not in null else None
    st = sc = None
    sbytes = 0
    if "stats" in has and "stats" not in null:
        st = c.out("stats", (1, 2, I32))
        sbytes = int(lib.maxk_topk_stats_scratch_bytes(n))
        sc = c.out("stats_scratch", sbytes)
    rec, rb, used = None, 0, 0
    if "records" in has and "records" not in null:
        used = chunk_bytes(layout, k)
        rb = (used + 15) // 16 * 16 + 16      # bytes past the chunks stay unwritten: a gap
        rec = c.out("records", (m, used, U8, rb))
    dn, dstride = None, 0
    if "dense" in has:
        dstride = d + 5 if strided else d
        dn = c.out("dense", (m, d, F32, dstride))
    md, s = MODES.index(mode), stream()               # MAXK_TOPK_EXACT = 0, _REF_COMPAT = 1
    a_ds, a_is = (ds, is_) if strided else (0, 0)
    if entry == "cbsr":
        rc = lib.maxk_topk_cbsr(ptr(x), ptr(sd), ptr(si), n, d, k, md, s)
    elif entry == "count":
        rc = lib.maxk_topk_cbsr_count(ptr(x), ptr(sd), ptr(si), ptr(cnt), n, d, k, md, s)
    elif entry == "tables":
        rc = lib.maxk_topk_cbsr_tables(ptr(x), ptr(sd), a_ds, ptr(si), a_is, ptr(cnt), n, d, k,
                                       md, s)
    elif entry == "ex":
        rc = lib.maxk_topk_cbsr_ex(ptr(x), ptr(sd), a_ds, ptr(si), a_is, ptr(cnt), ptr(st),
                                   ptr(sc), sbytes, n, d, k, md, s)
    elif entry == "records":
        rc = lib.maxk_topk_cbsr_records(ptr(x), ptr(rec), rb, layout or 0, ptr(sd), a_ds, ptr(si),
                                        a_is, ptr(cnt), ptr(st), ptr(sc), sbytes, n, d, k, md, s)
    elif entry == "dropout":
        rc = lib.maxk_topk_cbsr_dropout(ptr(x), ptr(rec), rb, layout or 0, ptr(sd), a_ds, ptr(si),
                                        a_is, ptr(cnt), ptr(st), ptr(sc), sbytes, n, d, k, md, p,
                                        SEED, ROW_OFFSET, s)
    else:
        rc = lib.maxk_topk_cbsr_dense(ptr(x), ptr(dn), dstride if strided else 0, ptr(rec), rb,
                                      layout or 0, ptr(sd), a_ds, ptr(si), a_is, ptr(cnt), ptr(st),
                                      ptr(sc), sbytes, n, d, k, md, p, SEED, ROW_OFFSET, s)
    c.ok(rc)
    c.done()
    CASES["top-k"] += 1
    if n == 0:
        # nothing is written; the statistics pair alone is defined: all zero (the forward then
        # takes f64), so that a consumer never reads an undefined pair
        for name in c.arenas:
            if name == "stats":
                assert host(st).tolist() == [[0, 0]], what
            else:
                c.untouched(name)
        return
    if sd is not None:
        assert_written(c, "sp_data")
        assert_bits(c, "sp_data", ref["values"])
    if si is not None:
        assert_bits(c, "sp_index", ref["index"])
    if cnt is not None:
        assert_bits(c, "count", ref["count"][None, :])
    if st is not None:
        assert_bits(c, "stats", ref["stats"][None, :])
    if rec is not None:
        assert_bits(c, "records", ref["records"][layout])
    if dn is not None:
        assert_written(c, "dense")
        assert_bits(c, "dense", ref["dense"])


@pytest.mark.parametrize("poison", POISONS, ids=hex)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", TOPK_ENTRIES)
def test_topk_outputs(gpu, entry, mode, poison):
    """Every top-k entry point, contiguous and (where it takes strides) with data_stride =
    k + 3, index_stride = k + 1 and dense_stride = D + 5: the header asks for element alignment
    only, so these are legal, and the gaps must survive."""
    for n in TOPK_N:
        for d, k in TOPK_DK:
            layouts = layouts_for(k) if "records" in HAS[entry] else [None]
            if entry != "records":
                layouts = layouts[:1]
            for layout in layouts:
                for strided in ((False, True) if "strides" in HAS[entry] else (False,)):
                    run_topk(gpu, poison, entry, mode, n, d, k, strided, layout=layout)


@pytest.mark.parametrize("poison", POISONS, ids=hex)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", sorted(NULLS))
def test_topk_nullable_outputs_in_turn(gpu, entry, mode, poison):
    for n in (5, 67):
        for d, k in TOPK_DK:
            for null in NULLS[entry]:
                run_topk(gpu, poison, entry, mode, n, d, k, False, null=frozenset(null),
                         layout=layouts_for(k)[0])


@pytest.mark.parametrize("poison", POISONS, ids=hex)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", TOPK_ENTRIES)
def test_topk_no_rows_writes_nothing(gpu, entry, mode, poison):
    """N = 0 with buffers that could hold five rows: no byte of any output changes, except the
    statistics pair, which is defined to be all zero."""
    for d, k in ((256, 16), (7, 3)):
        for strided in ((False, True) if "strides" in HAS[entry] else (False,)):
            run_topk(gpu, poison, entry, mode, 0, d, k, strided, layout=layouts_for(k)[0], rows=5)


# =========================================================================== scatter
SCATTER_N = [1, 5, 67]
SCATTER_DK = [(256, 16), (256, 128), (100, 16), (99, 10), (1, 1)]
SCATTER_ENTRIES = ["plain", "tables", "dropout", "merge", "merge_no_grad_sp",
                   "merge_no_grad_dense"]
_SCATTER_IN = {}


def scatter_inputs(n, d, k, repeated):
    key = (n, d, k, repeated)
    if key not in _SCATTER_IN:
        if repeated:   # few distinct features: most rows name one several times
            oi = np.random.default_rng(4).integers(0, min(d, 6), size=(n, k)).astype(np.uint8)
        else:
            oi = oracle.maxk(graphs.features(n, d, seed=11 + k).numpy(), k)[1]
        _SCATTER_IN[key] = (oi, graphs.features(n, k, seed=12 + k).numpy(),
                            graphs.features(n, d, seed=13 + k).numpy())
    return _SCATTER_IN[key]


def run_scatter(gpu, poison, entry, n, d, k, p, repeated=False):
    oi, gs, gd = scatter_inputs(n, d, k, repeated)
    what = f"scatter {entry} N={n} D={d} k={k} p={p} repeated={repeated} poison={poison:#x}"
    c = Call(gpu, poison, what)
    gin = c.out("grad_in", (n, d, F32))
    s = stream()
    g_sp = None if entry == "merge_no_grad_sp" else c.inp("grad_sp", gs)
    if entry == "tables":      # the selectors of interleaved records: row stride 5k, offset 4k
        table = np.full((n, 5 * k), 0xA5, np.uint8)
        table[:, 4 * k:] = oi
        sel = c.inp("sp_index", table)[:, 4 * k:]
        istride = 5 * k
    else:
        sel, istride = c.inp("sp_index", oi), 0
    if entry == "plain":
        c.ok(lib.maxk_scatter_backward(ptr(g_sp), ptr(sel), ptr(gin), n, d, k, s))
        want = oracle.maxk_backward(gs, oi, d)
    elif entry == "tables":
        c.ok(lib.maxk_scatter_backward_tables(ptr(g_sp), ptr(sel), istride, ptr(gin), n, d, k, s))
        want = oracle.maxk_backward(gs, oi, d)
    elif entry == "dropout":
        c.ok(lib.maxk_scatter_backward_dropout(ptr(g_sp), ptr(sel), 0, ptr(gin), n, d, k, p, SEED,
                                               ROW_OFFSET, s))
        want = merge_rows(gs, oi, None, p, SEED, ROW_OFFSET, D=d)
    else:
        g_dn, dstride = None, 0
        if entry != "merge_no_grad_dense":   # a row-strided grad_dense
            wide = np.full((n, d + 5), np.nan, np.float32)
            wide[:, :d] = gd
            g_dn, dstride = c.inp("grad_dense", wide), d + 5
        c.ok(lib.maxk_scatter_backward_merge(ptr(g_sp), ptr(sel), 0, ptr(g_dn), dstride, ptr(gin),
                                             n, d, k, p, SEED, ROW_OFFSET, s))
        want = merge_rows(None if g_sp is None else gs, oi, None if g_dn is None else gd, p, SEED,
                          ROW_OFFSET, D=d)
    c.done()
    CASES["scatter"] += 1
    assert_written(c, "grad_in")
    assert_bits(c, "grad_in", want)
    unselected = np.ones((n, d), bool)
    unselected[np.arange(n)[:, None], oi] = False
    assert not host(gin).view(np.uint32)[unselected].any(), f"{what}: unselected feature not +0.0"


@pytest.mark.parametrize("poison", POISONS, ids=hex)
@pytest.mark.parametrize("entry", SCATTER_ENTRIES)
def test_scatter_outputs(gpu, entry, poison):
    ps = (0.0,) if entry in ("plain", "tables") else (0.5,) if entry == "dropout" else (0.0, 0.5)
    for p in ps:
        for n in SCATTER_N:
            for d, k in SCATTER_DK:
                run_scatter(gpu, poison, entry, n, d, k, p)
        run_scatter(gpu, poison, entry, 9, 64, 8, p, repeated=True)   # the last slot wins
        run_scatter(gpu, poison, entry, 67, 256, 16, p, repeated=True)


@pytest.mark.parametrize("poison", POISONS, ids=hex)
def test_scatter_no_rows_writes_nothing(gpu, poison):
    c = Call(gpu, poison, f"scatter N=0 poison={poison:#x}")
    gin = c.out("grad_in", (5, 64, F32))
    g = c.inp("grad_sp", np.ones((5, 8), np.float32))
    sel = c.inp("sp_index", np.zeros((5, 8), np.uint8))
    gd = c.inp("grad_dense", np.ones((5, 64), np.float32))
    s = stream()
    c.ok(lib.maxk_scatter_backward(ptr(g), ptr(sel), ptr(gin), 0, 64, 8, s))
    c.ok(lib.maxk_scatter_backward_tables(ptr(g), ptr(sel), 0, ptr(gin), 0, 64, 8, s))
    c.ok(lib.maxk_scatter_backward_dropout(ptr(g), ptr(sel), 0, ptr(gin), 0, 64, 8, 0.5, 1, 0, s))
    c.ok(lib.maxk_scatter_backward_merge(ptr(g), ptr(sel), 0, ptr(gd), 0, ptr(gin), 0, 64, 8, 0.5,
                                         1, 0, s))
    c.done()
    c.untouched("grad_in")
    CASES["scatter"] += 4


# =========================================================================== graphs and plans
def rect_graph(rows, cols, seed):
    """rows x cols CSR: a full row, an empty row, random subsets of the columns."""
    rng = np.random.default_rng(seed)
    lists = [np.sort(rng.choice(cols, size=rng.integers(0, min(cols, 40) + 1), replace=False))
             for _ in range(rows)]
    lists[0] = np.arange(cols)
    lists[-1] = np.arange(0)
    p = np.zeros(rows + 1, np.int32)
    p[1:] = np.cumsum([len(x) for x in lists])
    ix = np.concatenate(lists).astype(np.int32)
    return p, ix, rng.standard_normal(ix.size).astype(np.float32)


ALL_GRAPHS = list(GRAPHS) + ["rect_5x70", "rect_70x5"]
_GRAPH, _FWD_REF, _BWD_REF = {}, {}, {}


def graph(name):
    """(p, ix, v, rows, cols), built once."""
    if name not in _GRAPH:
        if name.startswith("rect_"):
            rows, cols = (int(t) for t in name[5:].split("x"))
            _GRAPH[name] = rect_graph(rows, cols, rows) + (rows, cols)
        else:
            p, ix, v = GRAPHS[name]()
            _GRAPH[name] = (p, ix, v, p.size - 1, p.size - 1)
    return _GRAPH[name]


def squared(name):
    """The oracle is square: ptr padded with edgeless rows to n = max(rows, cols)."""
    p, ix, v, rows, cols = graph(name)
    n = max(rows, cols)
    pp = np.full(n + 1, p[-1], np.int32)
    pp[:rows + 1] = p
    return pp, ix, v, n


def pad_rows(a, n):
    out = np.zeros((n,) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out


def tables_for(name, d, k):
    cols = graph(name)[4]
    return oracle.maxk(graphs.features(cols, d, seed=k).numpy(), k)


def fwd_ref(name, d, k):
    """(od, oi, ref, mag) of the forward, per (graph, D, k)."""
    key = (name, d, k)
    if key not in _FWD_REF:
        rows = graph(name)[3]
        pp, ix, v, n = squared(name)
        od, oi = tables_for(name, d, k)
        ref, mag = oracle.spgemm_forward(pp, ix, v, pad_rows(od, n), pad_rows(oi, n), d,
                                         with_mag=True)
        _FWD_REF[key] = (od, oi, ref[:rows], mag[:rows])
    return _FWD_REF[key]


def bwd_ref(name, d, k):
    """(oi, g, ref, mag) of the backward, per (graph, D, k)."""
    key = (name, d, k)
    if key not in _BWD_REF:
        rows, cols = graph(name)[3:]
        pp, ix, v, n = squared(name)
        oi = tables_for(name, d, k)[1]
        g = graphs.features(rows, d, seed=k + 1).numpy()
        ref, mag = oracle.sspmm_backward(pp, ix, v, pad_rows(g, n), pad_rows(oi, n), with_mag=True)
        _BWD_REF[key] = (oi, g, ref[:cols], mag[:cols])
    return _BWD_REF[key]


def make_plan(c, name, d, k, opts):
    """An external-workspace plan (GraphPlan always builds one) over graph tensors that are
    inputs of the call."""
    p, ix, v, rows, cols = graph(name)
    dp, di, dv = c.inp("ptr", p), c.inp("idx", ix), c.inp("val", v)
    plan = mk.GraphPlan(dp, di, dv, rows, ix.size, d, k, num_cols=cols, options=opts)
    assert plan.external
    return plan, (plan.handle, ptr(dp), ptr(di), ptr(dv))


def ids_of(case):
    return ",".join(str(x) if not isinstance(x, dict) else
                    ("default" if not x else "+".join(f"{a}={b}" for a, b in x.items()))
                    for x in case)


# =========================================================================== forward
# (D, k, options, fwd_layout, fwd_fixed; neither depends on the graph): every layout in fixed
# point and in f64. Layout 3 (k % 4 != 0, k > 192: one feature per lane) has no fixed-point
# kernel, a request for one runs f64.
FWD_CASES = [
    (256, 8, {}, 2, 0), (256, 16, {}, 4, 1), (256, 32, {}, 0, 1),
    (256, 32, {"fwd_two_tables": 2}, 1, 1),
    (256, 250, {}, 3, 0), (256, 255, {}, 3, 0), (256, 250, {"fwd_fixed": 1}, 3, 0),
    (256, 16, {"fwd_fixed": 2}, 4, 0), (256, 32, {"fwd_fixed": 2}, 0, 0),
    (256, 32, {"fwd_two_tables": 2, "fwd_fixed": 2}, 1, 0),
    (256, 8, {"fwd_fixed": 1}, 2, 1), (256, 16, {"fwd_chunk3": 1}, 2, 1),
    (256, 16, {"fwd_tile_rows": 1}, 4, 1), (256, 16, {"fwd_tile_rows": 39}, 4, 1),
]


def check_forward(c, out, name, d, k, prior):
    _, _, ref, mag = fwd_ref(name, d, k)
    got = host(out)
    if prior is None:            # accumulate = 0: the whole of out is written
        assert_written(c, "out")
        assert_bar(c, got, ref, mag, "out")
        return
    p = graph(name)[0]
    has = np.diff(p) > 0
    assert_bar(c, got[has], prior[has].astype(np.float64) + ref[has], mag[has] + np.abs(prior[has]),
               "out (rows with edges, accumulated)")
    assert np.array_equal(got[~has].view(np.uint32), prior[~has].view(np.uint32)), \
        f"{c.what}: an edgeless row changed under accumulate = 1"


@pytest.mark.parametrize("case", FWD_CASES, ids=ids_of)
@pytest.mark.parametrize("name", ALL_GRAPHS)
def test_forward_outputs(gpu, name, case):
    d, k, opts, layout, fixed = case
    _, ix, _, rows, cols = graph(name)
    od, oi, _, _ = fwd_ref(name, d, k)
    prior = graphs.features(rows, d, seed=7).numpy()
    for poison in POISONS:
        tag = f"forward {name} D={d} k={k} {opts} poison={poison:#x}"
        c = Call(gpu, poison, tag)
        plan, g = make_plan(c, name, d, k, opts)
        info = plan.info()
        assert info["fwd_layout"] == layout, (tag, info["fwd_layout"])
        assert info["fwd_fixed"] == fixed, (tag, info["fwd_fixed"])
        SEEN["fwd"].add((info["fwd_layout"], info["fwd_fixed"]))
        fb = plan.fwd_ws_bytes
        sd, si = c.inp("sp_data", od), c.inp("sp_index", oi)
        E, s = ix.size, stream()

        def run(label, acc, launch):
            c.what = f"{tag} {label} accumulate={acc}"
            out = c.out("out", (rows, d, F32))
            ws = c.out("workspace", fb)       # exactly the reported size, dirty
            if acc:
                out.fill(torch.from_numpy(prior))
            c.ok(launch(out, ws, acc))
            c.done()
            check_forward(c, out, name, d, k, prior if acc else None)
            CASES["forward"] += 1
            SEEN["accumulate"].add(acc)

        for acc in (0, 1):
            run("_ws", acc, lambda out, ws, acc: lib.maxk_spgemm_forward_ws(
                *g, ptr(sd), ptr(si), ptr(out), rows, E, k, d, acc, ptr(ws), fb, s))
        # the statistics pair handed in (computed into an arena of its own, then an input)
        st = c.out("stats", (1, 2, I32))
        c.ok(lib.maxk_cbsr_stats(ptr(sd), ptr(si), cols, k, ptr(st), s))
        c.done()
        assert_bits(c, "stats", stats_pair(od)[None, :])
        pair = c.inp("stats_in", st.payload.clone())
        for acc in (1, 0):
            run("_ex", acc, lambda out, ws, acc: lib.maxk_spgemm_forward_ex(
                *g, ptr(sd), ptr(si), ptr(out), rows, E, k, d, acc, ptr(pair), 1, 0, ptr(ws), fb,
                s))
        # row-strided tables (element alignment only)
        wd = np.full((cols, k + 3), np.float32(np.nan), np.float32)
        wd[:, :k] = od
        wi = np.full((cols, k + 1), 0xA5, np.uint8)
        wi[:, :k] = oi
        tsd, tsi = c.inp("sp_data strided", wd), c.inp("sp_index strided", wi)
        run("_tables", 0, lambda out, ws, acc: lib.maxk_spgemm_forward_tables(
            *g, ptr(tsd), k + 3, ptr(tsi), k + 1, ptr(out), rows, E, k, d, acc, None, 0, 0,
            ptr(ws), fb, s))
        if layout in (1, 2, 4) and cols > 0:
            rb = info["fwd_record_bytes"]
            rec = c.inp("records", pack_records(sd, si, layout, rb))
            fb = 0                            # _records takes no workspace
            for acc in (0, 1):
                run("_records", acc, lambda out, ws, acc: lib.maxk_spgemm_forward_records(
                    *g, ptr(rec), rb, layout, ptr(out), rows, E, k, d, acc, ptr(pair), 1, 0, s))


# =========================================================================== backward
BWD_OPTIONS = [
    {}, {"bwd_algo": 3}, {"bwd_algo": 3, "bwd_tp_chunks": 2}, {"bwd_algo": 3, "bwd_tp_chunks": 5},
    {"bwd_tasks_per_cu": 64, "bwd_min_task_edges": 16},
    {"bwd_tasks_per_cu": 64, "bwd_min_task_edges": 16, "bwd_flush": 1},
    {"bwd_piece_edges": 500}, {"bwd_features_per_lane": 2}, {"bwd_slot_groups": 2},
    {"bwd_slot_groups": 4}, {"col_order": "scattered"}, {"bwd_row_order": 2},
]
# every knob value here is one the parity suite's PLAN_OPTIONS runs too
assert all(any(q.get(a) == b for q in PLAN_OPTIONS) for o in BWD_OPTIONS for a, b in o.items())
# k that is no multiple of the slots per lane F (the last row's padding slots sit next to the
# trailing guard), at the default F, F = 4 and F = 2
BWD_PADDED = [(256, 1), (256, 7), (256, 13), (64, 17), (256, 255)]
BWD_CASES = ([(256, k, o) for o in BWD_OPTIONS for k in (16, 32)] +
             [(d, k, {"bwd_algo": 1, **({"bwd_features_per_lane": f} if f else {})})
              for d, k in BWD_PADDED for f in (0, 4, 2)])


@pytest.mark.parametrize("case", BWD_CASES, ids=ids_of)
@pytest.mark.parametrize("name", ALL_GRAPHS)
def test_backward_outputs(gpu, name, case):
    d, k, opts = case
    _, ix, _, rows, cols = graph(name)
    oi, g, ref, mag = bwd_ref(name, d, k)
    for poison in POISONS:
        tag = f"backward {name} D={d} k={k} {opts} poison={poison:#x}"
        c = Call(gpu, poison, tag)
        plan, gr = make_plan(c, name, d, k, opts)
        info = plan.info()
        SEEN["bwd_algo"].add(info["bwd_algo"])
        if opts.get("bwd_algo") == 3:
            assert info["bwd_algo"] == (3 if ix.size else 1), tag
        if opts.get("bwd_algo") == 1:
            assert info["bwd_algo"] == 1, tag
        if "bwd_min_task_edges" in opts and name == "heavy_split" and k == 16:
            assert info["bwd_shared_blocks"] > 0 and (plan.bwd_ws_bytes > 0) == \
                (opts.get("bwd_flush", 2) == 2), tag     # the slab regions are in play
        bb = plan.bwd_ws_bytes
        go, si = c.inp("grad_out", g), c.inp("sp_index", oi)
        wide = np.full((cols, 5 * k), 0xA5, np.uint8)   # interleaved records: index_stride 5k
        wide[:, 4 * k:] = oi
        wsel = c.inp("sp_index strided", wide)[:, 4 * k:]
        E, s = ix.size, stream()
        for label in ("_ws", "_tables"):
            c.what = f"{tag} {label}"
            gs = c.out("grad_sp", (cols, k, F32))
            ws = c.out("workspace", bb)       # exactly the reported size, dirty
            if label == "_ws":
                c.ok(lib.maxk_sspmm_backward_ws(*gr, ptr(go), ptr(si), ptr(gs), rows, E, k, d,
                                                ptr(ws), bb, s))
            else:
                c.ok(lib.maxk_sspmm_backward_tables(*gr, ptr(go), ptr(wsel), 5 * k, ptr(gs), rows,
                                                    E, k, d, ptr(ws), bb, s))
            c.done()
            assert_written(c, "grad_sp")
            assert_bar(c, host(gs), ref, mag, "grad_sp")
            CASES["backward"] += 1


# =========================================================================== dense SpMM, statistics
@pytest.mark.parametrize("poison", POISONS, ids=hex)
@pytest.mark.parametrize("dim", [4, 100, 256, 512])
@pytest.mark.parametrize("name", ["empty_rows", "no_edges", "heavy_split"])
def test_dense_spmm_output(gpu, name, dim, poison):
    """Y in an arena, against the f64-accumulating oracle: X taken 256 columns at a time as a
    CBSR table that selects every feature."""
    p, ix, v, n, _ = graph(name)
    x = graphs.features(n, dim, seed=dim).numpy()
    ref, mag = np.empty((n, dim), np.float32), np.empty((n, dim), np.float32)
    for c0 in range(0, dim, 256):
        w = min(256, dim - c0)
        sel = np.broadcast_to(np.arange(w, dtype=np.uint8), (n, w))
        ref[:, c0:c0 + w], mag[:, c0:c0 + w] = oracle.spgemm_forward(
            p, ix, v, x[:, c0:c0 + w], sel, w, with_mag=True)
    c = Call(gpu, poison, f"dense SpMM {name} dim={dim} poison={poison:#x}")
    dp, di, dv, dx = c.inp("ptr", p), c.inp("idx", ix), c.inp("val", v), c.inp("X", x)
    y = c.out("Y", (n, dim, F32))
    c.ok(lib.maxk_dense_spmm_csr(ptr(dp), ptr(di), ptr(dv), ptr(dx), ptr(y), n, dim, stream()))
    c.done()
    assert_written(c, "Y")
    assert_bar(c, host(y), ref, mag, "Y")
    CASES["dense and statistics"] += 1


@pytest.mark.parametrize("poison", POISONS, ids=hex)
@pytest.mark.parametrize("mode", MODES)
def test_cbsr_stats_output(gpu, mode, poison):
    """The two words of maxk_cbsr_stats / _tables in an arena (no third word is touched), on
    tables of 0 to 3000 rows, plain and row-strided."""
    for n, d, k in ((0, 64, 8), (1, 1, 1), (5, 100, 5), (67, 256, 16), (3000, 256, 66)):
        od, oi = oracle.maxk(graphs.features(max(n, 1), d, seed=n + k).numpy(), k, mode)
        od, oi = od[:n], oi[:n]
        for strided in (False, True):
            c = Call(gpu, poison, f"cbsr_stats {mode} N={n} k={k} strided={strided} "
                                  f"poison={poison:#x}")
            st = c.out("stats", (1, 2, I32))
            if strided:
                wd = np.full((n, k + 3), np.float32(np.nan), np.float32)
                wd[:, :k] = od
                wi = np.full((n, k + 1), 0xA5, np.uint8)
                wi[:, :k] = oi
                sd, si = c.inp("sp_data", wd), c.inp("sp_index", wi)
                c.ok(lib.maxk_cbsr_stats_tables(ptr(sd), k + 3, ptr(si), k + 1, n, k, ptr(st),
                                                stream()))
            else:
                sd, si = c.inp("sp_data", od), c.inp("sp_index", oi)
                c.ok(lib.maxk_cbsr_stats(ptr(sd), ptr(si), n, k, ptr(st), stream()))
            c.done()
            assert_bits(c, "stats", stats_pair(od)[None, :])
            CASES["dense and statistics"] += 1


# =========================================================================== autograd
_STEP_REF = {}


def step_ref(name, d, k, mode, p_drop):
    """Oracle references of one training step on (graph, k, mode, p): the dense masked row, the
    aggregate, and the input gradients of maxk_aggregate (aggregate alone) and
    maxk_self_aggregate (both outputs)."""
    key = (name, d, k, mode, p_drop)
    if key in _STEP_REF:
        return _STEP_REF[key]
    p, ix, v, n, _ = graph(name)
    x = graphs.features(n, d, seed=31 + k)
    g_agg = graphs.features(n, d, seed=32 + k)
    g_self = graphs.features(n, d, seed=33 + k)
    od, oi = oracle.maxk(x.numpy(), k, mode)
    odd = dropped_table(od, oi, p_drop, SEED) if p_drop else od
    cnt = _filled_count(od, oi) if mode == "ref_compat" else None
    xm = dense_rows(odd, oi, cnt, d)
    y, ymag = oracle.spgemm_forward(p, ix, v, odd, oi, d, with_mag=True)
    gs, gmag = oracle.sspmm_backward(p, ix, v, g_agg.numpy(), oi, with_mag=True)
    scale = float(drop_scale(p_drop)) if p_drop else 1.0
    keep = keep_mask(p_drop, SEED, np.arange(n)[:, None], oi) if p_drop else np.ones_like(oi, bool)
    filled = (np.arange(k)[None, :] < cnt[:, None]) if cnt is not None else np.ones_like(od, bool)
    rows = np.repeat(np.arange(n)[:, None], k, 1)

    def scattered(vals):
        out = np.zeros((n, d))
        out[rows[filled], oi[filled]] = vals[filled]
        return out

    gk = np.take_along_axis(g_self.numpy().astype(np.float64), oi.astype(np.int64), 1)
    _STEP_REF[key] = dict(
        x=x, g_agg=g_agg, g_self=g_self, xm=xm, y=y, ymag=ymag,
        gx_agg=scattered(gs.astype(np.float64) * keep * scale),
        gx_agg_mag=scattered(gmag.astype(np.float64) * scale),
        gx_both=scattered((gs.astype(np.float64) + gk) * keep * scale),
        gx_both_mag=scattered((gmag.astype(np.float64) + np.abs(gk)) * scale))
    return _STEP_REF[key]


def train_step(gpu, gr, ref, k, mode, p_drop, self_term):
    xg = ref["x"].to(gpu).requires_grad_(True)
    if self_term:
        xm, y = mk.maxk_self_aggregate(xg, gr, k, mode, dropout_p=p_drop, seed=SEED)
        torch.autograd.backward([xm, y], [ref["g_self"].to(gpu), ref["g_agg"].to(gpu)])
    else:
        xm, y = None, mk.maxk_aggregate(xg, gr, k, mode, dropout_p=p_drop, seed=SEED)
        y.backward(ref["g_agg"].to(gpu))
    torch.cuda.synchronize()
    return xm, y.detach(), xg.grad


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [8, 16, 32])
@pytest.mark.parametrize("name", ["heavy_split", "empty_rows"])
def test_autograd_path_on_dirty_workspaces(gpu, monkeypatch, name, k, mode, p_drop):
    """maxk_aggregate and maxk_self_aggregate, forward and backward, with GraphPlan._workspace
    handing out poisoned arenas of exactly the requested size: the same step as with torch's
    allocator (bit-equal where the forward runs fixed point, the oracle bar for both runs),
    and every arena handed out is intact."""
    d = 256
    p, ix, v, n, _ = graph(name)
    ref = step_ref(name, d, k, mode, p_drop)
    gr = mk.CSRGraph(*(torch.from_numpy(a).to(gpu) for a in (p, ix, v)))
    fixed = gr.plan(d, k).fwd_fixed
    # rows split over several work-groups meet in f32 global atomics, whose order varies
    whole = torch.from_numpy(np.diff(p) < n).to(gpu) if name == "heavy_split" else slice(None)
    assert gr.plan(d, k).info()["fwd_split_rows"] == (2 if name == "heavy_split" else 0)
    c = Call(gpu, 0, f"autograd {name} k={k} {mode} p={p_drop}")

    def checked(run, self_term):
        xm, y, gx = run
        if self_term:
            assert np.array_equal(xm.detach().cpu().numpy().view(np.uint32),
                                  ref["xm"].view(np.uint32)), c.what
        assert_bar(c, y.cpu().numpy(), ref["y"], ref["ymag"], "aggregate")
        which = "gx_both" if self_term else "gx_agg"
        assert_bar(c, gx.cpu().numpy(), ref[which], ref[which + "_mag"], "input gradient")
        return run

    for self_term in (False, True):
        plain = checked(train_step(gpu, gr, ref, k, mode, p_drop, self_term), self_term)
        for poison in POISONS:
            c.what = f"autograd {name} k={k} {mode} p={p_drop} self={self_term} poison={poison:#x}"
            handed = []

            def workspace(plan, nbytes, poison=poison, handed=handed):
                if not plan.external or nbytes == 0:
                    return None, 0
                handed.append(Arena(nbytes, plan.device, poison))
                return handed[-1].payload, nbytes

            with monkeypatch.context() as m:
                m.setattr(mk.GraphPlan, "_workspace", workspace)
                dirty = checked(train_step(gpu, gr, ref, k, mode, p_drop, self_term), self_term)
            SEEN["autograd_arenas"] += len(handed)   # none at k = 8, 16: records, unsplit blocks
            for i, a in enumerate(handed):
                assert a.check() is None, f"{c.what}: write outside workspace {i}: {a.check()}"
            if fixed:
                assert torch.equal(dirty[1][whole], plain[1][whole]), f"{c.what}: aggregate differs"
            CASES["autograd"] += 1
    mk.clear_plan_cache()


# =========================================================================== what ran
def test_contract_coverage_report(gpu):
    """Runs last (file order): how many cases each family ran, and that no kernel path dropped
    out: forward layouts 0 to 4 in fixed point and in f64 (layout 3 has f64 only), both
    accumulations, both backward algorithms."""
    if not all(CASES.values()):
        pytest.skip("not every family ran in this session (-k selection)")
    for family, count in CASES.items():
        print(f"contracts: {family}: {count} cases")
    print(f"contracts: (fwd_layout, fwd_fixed) seen: {sorted(SEEN['fwd'])}; accumulate: "
          f"{sorted(SEEN['accumulate'])}; bwd_algo: {sorted(SEEN['bwd_algo'])}; workspaces handed "
          f"to autograd steps: {SEEN['autograd_arenas']}; "
          f"{time.time() - T0:.0f} s since the module was imported")
    want = {(l, f) for l in (0, 1, 2, 4) for f in (0, 1)} | {(3, 0)}
    assert SEEN["fwd"] >= want, sorted(want - SEEN["fwd"])
    assert SEEN["accumulate"] == {0, 1} and SEEN["bwd_algo"] >= {1, 3}
    assert SEEN["autograd_arenas"] > 0, "no autograd step took a workspace: nothing was poisoned"
