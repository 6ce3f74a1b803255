"""GPU: every k (and every D) through every kernel class, bit for bit, on the exact inputs of
tests/sweep.py (their preconditions are checked on the CPU in tests/test_sweep_inputs.py).

1. plan kernels, every k in 1..256 at D = 256 on both graphs with default options;
2. the same sweep on the sparse graph with one explicit option at a time, each plan held to
   sweep.expected (what include/maxk_hip.h documents: accepted, fallback or refusal);
3. every D in 1..256 with k in {1, ceil(D / 2), D} through the entry points the fuzz uses;
4. the top-k in both modes at 16 widths and every k, and at D = 256 every k through the record
   layouts, the fused dropout, the dense row and the fused statistics pair;
5. the three scatters; 6. the SDDMM; 7. maxk_aggregate and maxk_self_aggregate;
8. a coverage report: every case ran, the refusals are exactly the table's, every documented
   plan_info value appeared (printed with -s).

Sums are compared with np.array_equal against the oracle's f64 results (every term is a multiple
of 0.5 and the sums stay below 2^22, so any order is exact in f32); the top-k, its variants and
the scatters are compared as bit patterns with the oracle and the numpy restatements of
test_records_capi / test_dropout_capi / test_self_capi / test_edge_grad_capi.
"""
import collections
import ctypes
import functools
import re
import time

import numpy as np
import pytest
import torch

import maxk_kernels as mk
import sweep
from maxk_kernels import _lib
from oracle import oracle
from test_dropout_capi import dropped_table
from test_edge_grad_capi import edge_grad_rows
from test_gpu_contracts import stats_pair
from test_gpu_parity import graph_on, to_dev
from test_gpu_records import SENTINEL, pack_records
from test_self_capi import dense_rows, merge_rows

pytestmark = pytest.mark.gpu

N, D = sweep.N, sweep.D_FULL
DROP = (sweep.DROP_P, sweep.SEED, sweep.ROW_OFFSET)
P = ctypes.c_void_p

RECORD = {}                                   # case key -> "ok" | "refused"
INFOS = collections.defaultdict(list)         # (graph, option id) -> [(k, info fields)]
STARTED = set()                               # parametrized blocks that began
SECONDS = collections.Counter()               # wall time per section
INFO_FIELDS = ("fwd_layout", "fwd_fixed", "fwd_waves", "fwd_unroll", "bwd_algo", "bwd_waves",
               "bwd_unroll", "bwd_blocks", "bwd_tasks", "fwd_split_rows")
# the dense graph last: the sparse references of a block of k stay cached across the option sets
PLAN_BLOCKS = ([("sparse", "default")] +
               [("sparse", sweep.opt_id(o)) for o in sweep.OPTION_SETS] + [("dense", "default")])
# blocks of 32 k of the plan sweep and of six more tests, one per width of the top-k, and the
# scatters' widths
N_BLOCKS = (len(PLAN_BLOCKS) + 6) * len(sweep.BLOCKS) + len(sweep.D_LIST) + 1


class section:
    """Marks a parametrized block as started and adds its wall time to its section."""

    def __init__(self, name, *block):
        self.name, self.block = name, (name,) + block

    def __enter__(self):
        STARTED.add(self.block)
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        SECONDS[self.name] += time.perf_counter() - self.t0


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else a.dtype)


def assert_exact(got, ref, what):
    """np.array_equal against the oracle's sums, with the first difference in the message."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    ref = np.asarray(ref).astype(np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = got != ref
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at "
                             f"{at}: got {got[bad][:4]}, oracle {ref[bad][:4]}")


def assert_bits(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if not np.array_equal(g, r):
        bad = g != r
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bit patterns differ, first "
                             f"at {at}: got {g[bad][:4]}, expected {r[bad][:4]}")


@functools.lru_cache(maxsize=None)
def dev_graph(gpu, gname):
    return graph_on(gpu, *sweep.graph(gname))


@functools.lru_cache(maxsize=40)
def dev_case(gpu, gname, d, k):
    """(oracle table values, selectors, gradient) of an exact case on the device."""
    c = sweep.case(gname, d, k)
    return to_dev(c.od, gpu), to_dev(c.oi, gpu), to_dev(c.g, gpu)


# ------------------------------------------------------------------ 1, 2: plan kernels
def run_plan_case(gpu, gname, k, oid):
    key = ("plan", gname, k, oid)
    opts = sweep.OPTIONS[oid]
    exp = sweep.expected(gname, k, opts)
    c = sweep.case(gname, D, k)
    ptr, idx, val = dev_graph(gpu, gname)
    try:
        plan = mk.GraphPlan(ptr, idx, val, N, c.ix.size, D, k, options=opts)
    except _lib.MaxKError as exc:            # only a documented refusal passes
        code = int(re.search(r"code (-?\d+)", str(exc)).group(1))
        assert exp.kind == "refused" and code == exp.code, (key, str(exc))
        RECORD[key] = "refused"
        return
    assert exp.kind != "refused", (key, "the header documents a refusal", exp.code)
    info = plan.info()
    wrong = {f: (info[f], v) for f, v in exp.info.items() if info[f] != v}
    assert not wrong, f"{key}: plan_info (got, documented) {wrong}; {exp.kind} {exp.note}"
    INFOS[(gname, oid)].append((k, tuple(info[f] for f in INFO_FIELDS)))
    od, oi, g = dev_case(gpu, gname, D, k)
    assert_exact(plan.forward(od, oi), c.fwd, f"{key} forward")
    assert_exact(plan.backward(g, oi), c.bwd, f"{key} backward")
    RECORD[key] = "ok"


@pytest.mark.parametrize("gname,oid", PLAN_BLOCKS, ids=[f"{g}-{o}" for g, o in PLAN_BLOCKS])
@pytest.mark.parametrize("lo,hi", sweep.BLOCKS)
def test_plan_kernels_every_k(gpu, lo, hi, gname, oid):
    """GraphPlan.forward / backward on the oracle's exact top-k table against
    oracle.spgemm_forward / sspmm_backward, and plan.info() against the header's table; a plan
    creation error the table does not predict fails the case. The option id varies fastest, so
    a block's 32 references are computed once."""
    with section("plan", lo, gname, oid):
        for k in range(lo, hi + 1):
            run_plan_case(gpu, gname, k, oid)


# ------------------------------------------------------------------ 3: every D
@pytest.mark.parametrize("lo,hi", sweep.BLOCKS)
def test_every_d_through_the_reference_functions(gpu, lo, hi):
    """spgemm_forward, spgemm_backward and maxk_backward (the fuzz's entry points, which accept
    every D) on the sparse graph."""
    ptr, idx, val = dev_graph(gpu, "sparse")
    with section("dsweep", lo):
        for d in range(lo, hi + 1):
            for k in sweep.d_sweep_ks(d):
                c = sweep.case("sparse", d, k)
                od, oi, g = to_dev(c.od, gpu), to_dev(c.oi, gpu), to_dev(c.g, gpu)
                out, _ = mk.spgemm_forward(ptr, idx, val, od, oi, N, c.ix.size, k, d)
                assert_exact(out, c.fwd, f"D={d} k={k} forward")
                gs = mk.spgemm_backward(ptr, idx, val, g, oi, N, c.ix.size, k, d)
                assert_exact(gs, c.bwd, f"D={d} k={k} backward")
                gin = mk.maxk_backward(gs, oi, dim_origin=d)
                assert_bits(gin, oracle.maxk_backward(c.bwd, c.oi, d), f"D={d} k={k} scatter")
                RECORD[("dsweep", d, k)] = "ok"
            mk.clear_plan_cache()


# ------------------------------------------------------------------ 4: top-k
@functools.lru_cache(maxsize=4)
def topk_ref(d, k, mode):
    x = sweep.topk_rows(d)
    od, oi = oracle.maxk(x, k, mode)
    return od, oi, sweep.topk_counts(x, k, mode)


@pytest.mark.parametrize("d", sweep.D_LIST)
def test_topk_every_k(gpu, d):
    """Values, selectors and counts of both modes against oracle.maxk on 40 rows: N(0, 1), ties,
    all equal, +-0, denormals, NaN and Inf (sweep.topk_rows)."""
    xt = to_dev(sweep.topk_rows(d), gpu)
    with section("topk", d):
        for k in range(1, d + 1):
            for mode in sweep.MODES:
                od, oi, cnt = topk_ref(d, k, mode)
                sd, si, sc = mk.maxk_forward(xt, k, mode=mode, return_index=True,
                                             return_count=True)
                what = f"D={d} k={k} {mode}"
                assert_bits(si, oi, what + " selectors")
                assert_bits(sd, od, what + " values")
                assert np.array_equal(sc.cpu().numpy(), cnt), (what, "counts")
            RECORD[("topk", d, k)] = "ok"


def refused_records_call(xt, rec, k, layout):
    """maxk_topk_cbsr_records with valid buffers and a layout the header does not allow at k:
    the return code (argument errors are reported before any device call)."""
    n = xt.shape[0]
    sd = torch.empty((n, k), device=xt.device)
    si = torch.empty((n, k), dtype=torch.uint8, device=xt.device)
    stream = P(torch.cuda.current_stream().cuda_stream)
    return _lib.lib.maxk_topk_cbsr_records(P(xt.data_ptr()), P(rec.data_ptr()), rec.shape[1],
                                           layout, P(sd.data_ptr()), 0, P(si.data_ptr()), 0, None,
                                           None, None, 0, n, xt.shape[1], k, 0, stream)


@pytest.mark.parametrize("lo,hi", sweep.BLOCKS)
def test_topk_records_every_k(gpu, lo, hi):
    """maxk_topk_cbsr_records at D = 256 in every layout: the record bytes of the layouts the
    header allows at k (packed on the CPU from the oracle's table, bytes past the record
    untouched), with the plain tables and counts, and on the finite rows the fused statistics
    pair; the documented refusal for the others."""
    x = sweep.topk_rows(D)
    xt = to_dev(x, gpu)
    fin = sweep.TOPK_FINITE
    big = torch.empty((40, 4096), dtype=torch.uint8, device=gpu)
    with section("records", lo):
        for k in range(lo, hi + 1):
            for layout in sweep.LAYOUTS:
                key = ("records", k, layout)
                code = sweep.records_expected(k, layout)
                if code != 0:
                    rc = refused_records_call(xt, big, k, layout)
                    assert rc == code, (key, rc, _lib.lib.maxk_last_error())
                    RECORD[key] = "refused"
                    continue
                used = sweep.record_chunk_bytes(layout, k)
                rb = (used + 15) // 16 * 16 + 32
                for mode in sweep.MODES:
                    od, oi, cnt = topk_ref(D, k, mode)
                    want = pack_records(torch.from_numpy(od), torch.from_numpy(oi), layout,
                                        rb).numpy()
                    rec = torch.full((40, rb), SENTINEL, dtype=torch.uint8, device=gpu)
                    sd, si, sc = mk.maxk_forward(xt, k, mode=mode, return_index=True,
                                                 return_count=True, records=(rec, layout))
                    what = f"{key} {mode}"
                    assert np.array_equal(rec.cpu().numpy(), want), what + " record bytes"
                    assert_bits(si, oi, what + " selectors")
                    assert_bits(sd, od, what + " values")
                    assert np.array_equal(sc.cpu().numpy(), cnt), what + " counts"
                    st = torch.full((2,), -1, dtype=torch.int32, device=gpu)
                    rec.fill_(SENTINEL)
                    mk.maxk_forward(xt[:fin], k, mode=mode, return_index=True,
                                    records=(rec[:fin], layout), stats=st)
                    assert st.tolist() == stats_pair(od[:fin]).tolist(), what + " statistics"
                    assert np.array_equal(rec[:fin].cpu().numpy(), want[:fin]), what
                RECORD[key] = "ok"


@pytest.mark.parametrize("lo,hi", sweep.BLOCKS)
def test_topk_dropout_dense_and_stats_every_k(gpu, lo, hi):
    """At D = 256: maxk_topk_cbsr_dropout (p = 0.5, row_offset 3) against the oracle's table
    through the numpy mask; maxk_topk_cbsr_dense with and without dropout against
    test_self_capi.dense_rows; maxk_topk_cbsr_ex's statistics pair on the finite rows."""
    x = sweep.topk_rows(D)
    xt = to_dev(x, gpu)
    fin = sweep.TOPK_FINITE
    with section("variants", lo):
        for k in range(lo, hi + 1):
            for mode in sweep.MODES:
                od, oi, cnt = topk_ref(D, k, mode)
                dropped = dropped_table(od, oi, *DROP)
                what = f"k={k} {mode}"
                st = torch.full((2,), -1, dtype=torch.int32, device=gpu)
                sd, si, sc = mk.maxk_forward(xt, k, mode=mode, return_index=True,
                                             return_count=True, dropout=DROP)
                assert_bits(sd, dropped, what + " dropout values")
                assert_bits(si, oi, what + " dropout selectors")
                assert np.array_equal(sc.cpu().numpy(), cnt), what + " dropout counts"
                mk.maxk_forward(xt[:fin], k, mode=mode, dropout=DROP, stats=st)
                assert st.tolist() == stats_pair(dropped[:fin]).tolist(), what + " dropout pair"
                for drop, table in ((None, od), (DROP, dropped)):
                    dense = torch.full((40, D), float("nan"), device=gpu)
                    sd, si = mk.maxk_forward(xt, k, mode=mode, return_index=True, dropout=drop,
                                             dense=dense)
                    assert_bits(dense, dense_rows(table, oi, cnt, D),
                                what + f" dense row, dropout {drop is not None}")
                    assert_bits(sd, table, what + " dense: values")
                    assert_bits(si, oi, what + " dense: selectors")
                st.fill_(-1)
                sd, si = mk.maxk_forward(xt[:fin], k, mode=mode, return_index=True, stats=st)
                assert st.tolist() == stats_pair(od[:fin]).tolist(), what + " statistics pair"
                assert_bits(sd, od[:fin], what + " stats: values")
            for name in ("dropout", "dense", "stats"):
                RECORD[(name, k)] = "ok"


# ------------------------------------------------------------------ 5: scatters
def run_scatter_case(gpu, d, k):
    """maxk_scatter_backward_tables, _dropout and _merge on 40 rows of N(0, 1) gradients with the
    oracle's selectors of both modes (ref_compat: repeated selector 0 in the padding slots, the
    last slot wins), against oracle.maxk_backward and test_self_capi.merge_rows."""
    rs = np.random.RandomState(7000 + 300 * d + k)
    gs = rs.randn(40, k).astype(np.float32)
    gd = rs.randn(40, d).astype(np.float32)
    gst, gdt = to_dev(gs, gpu), to_dev(gd, gpu)
    for mode in sweep.MODES:
        oi = oracle.maxk(sweep.topk_rows(d), k, mode)[1]
        sit = to_dev(oi, gpu)
        what = f"D={d} k={k} {mode}"
        assert_bits(mk.maxk_backward(gst, sit, dim_origin=d), oracle.maxk_backward(gs, oi, d),
                    what + " scatter")
        assert_bits(mk.maxk_backward(gst, sit, dim_origin=d, dropout=DROP),
                    merge_rows(gs, oi, None, *DROP, D=d), what + " dropout scatter")
        for drop, args in ((None, (0.0, 0, 0)), (DROP, DROP)):
            assert_bits(mk.maxk_backward(gst, sit, dim_origin=d, dropout=drop, grad_dense=gdt),
                        merge_rows(gs, oi, gd, *args, D=d), what + f" merge scatter {args[0]}")
    RECORD[("scatter", d, k)] = "ok"


@pytest.mark.parametrize("lo,hi", sweep.BLOCKS)
def test_scatters_every_k(gpu, lo, hi):
    with section("scatter", lo):
        for k in range(lo, hi + 1):
            run_scatter_case(gpu, D, k)


def test_scatters_every_width(gpu):
    with section("scatter", "widths"):
        for d in sweep.D_LIST[:-1]:
            for k in sweep.d_sweep_ks(d):
                run_scatter_case(gpu, d, k)


# ------------------------------------------------------------------ 6: SDDMM
@pytest.mark.parametrize("lo,hi", sweep.BLOCKS)
def test_sddmm_every_k(gpu, lo, hi):
    """maxk_sddmm_edge_grad on the sparse graph against the pinned tree's restatement
    (test_edge_grad_capi.edge_grad_rows): the exact inputs, where the tree also equals the f64
    sum, and the same with one gradient row and one table row of N(0, 1) values (the heavy row
    and its first source column), where only the pinned order gives the bits."""
    p, ix, _ = sweep.graph("sparse")
    ptr, idx, _ = dev_graph(gpu, "sparse")
    h = sweep.HEAVY_ROW["sparse"]
    col = int(ix[p[h]])
    with section("sddmm", lo):
        for k in range(lo, hi + 1):
            c = sweep.case("sparse", D, k)
            od, oi, g = dev_case(gpu, "sparse", D, k)
            got = mk.spgemm_edge_grad(ptr, idx, g, od, oi, N, ix.size, k, D)
            ref = edge_grad_rows(p, ix, c.g, c.od, c.oi)
            rows = np.repeat(np.arange(N), np.diff(p))
            f64 = (c.od[ix].astype(np.float64) * c.g[rows[:, None], c.oi[ix]]).sum(1)
            assert np.array_equal(ref, f64)
            assert_bits(got, ref, f"k={k} SDDMM, exact inputs")
            rs = np.random.RandomState(8000 + k)
            g2, od2 = c.g.copy(), c.od.copy()
            g2[h] = rs.randn(D)
            od2[col] = rs.randn(k)
            got = mk.spgemm_edge_grad(ptr, idx, to_dev(g2, gpu), to_dev(od2, gpu), oi, N, ix.size,
                                      k, D)
            assert_bits(got, edge_grad_rows(p, ix, g2, od2, c.oi), f"k={k} SDDMM, N(0, 1) rows")
            RECORD[("sddmm", k)] = "ok"


# ------------------------------------------------------------------ 7: autograd
@pytest.mark.parametrize("lo,hi", sweep.BLOCKS)
def test_aggregate_functions_every_k(gpu, lo, hi):
    """maxk_aggregate and maxk_self_aggregate in exact mode, p in {0, 0.5}, on the sparse graph:
    outputs and x.grad equal the exact case's references (the records path in whichever layout
    the plan picks for k). The self pair gets an integer gradient on its dense output too, which
    the merge scatter adds before the dropout scale: still exact."""
    graph = mk.CSRGraph(*dev_graph(gpu, "sparse"))
    rows = np.arange(N)[:, None]
    with section("autograd", lo):
        for k in range(lo, hi + 1):
            g_self = sweep.int_features(N, D, seed=3000 + k)
            for p in (0.0, sweep.DROP_P):
                c = sweep.case("sparse", D, k, p)
                g = to_dev(c.g, gpu)
                what = f"k={k} p={p}"
                x = to_dev(c.x, gpu).requires_grad_(True)
                y = mk.maxk_aggregate(x, graph, k, "exact", dropout_p=p, seed=sweep.SEED)
                y.backward(g)
                assert_exact(y, c.fwd, what + " maxk_aggregate")
                assert_exact(x.grad, c.gx, what + " maxk_aggregate x.grad")
                x = to_dev(c.x, gpu).requires_grad_(True)
                xm, y = mk.maxk_self_aggregate(x, graph, k, "exact", dropout_p=p, seed=sweep.SEED)
                torch.autograd.backward([xm, y], [to_dev(g_self, gpu), g])
                xm_ref = np.zeros((N, D), np.float32)
                xm_ref[rows, c.oi] = c.od                # exact mode: selectors never repeat
                assert_bits(xm, xm_ref, what + " maxk_self_aggregate dense")
                assert_exact(y, c.fwd, what + " maxk_self_aggregate")
                assert_bits(x.grad, merge_rows(c.bwd, c.oi, g_self, p, sweep.SEED, D=D),
                            what + " maxk_self_aggregate x.grad")
            RECORD[("autograd", k)] = "ok"
        mk.clear_plan_cache()


# ------------------------------------------------------------------ 8: coverage report
def k_ranges(ks):
    ks, out, i = sorted(ks), [], 0
    while i < len(ks):
        j = i
        while j + 1 < len(ks) and ks[j + 1] == ks[j] + 1:
            j += 1
        out.append(str(ks[i]) if i == j else f"{ks[i]}-{ks[j]}")
        i = j + 1
    return ",".join(out)


def test_sweep_coverage_report(gpu):
    """Runs last (file order). Every case of sweep.all_cases() ran: the full product minus
    exactly the table's refusals, none skipped (the cap on cases left out is zero); and every
    documented plan_info value appeared. bwd_waves: these graphs' default plans run the
    16-wave shape (counter hand-out, grad_out under 4 GiB), 8 and 12 come from the bwd_waves
    option sets; bwd_unroll 16 has no default and is not asked for."""
    if len(STARTED) < N_BLOCKS:
        pytest.skip(f"a -k selection ran {len(STARTED)} of {N_BLOCKS} blocks of the sweep")
    cases = sweep.all_cases()
    missing = [c for c in cases if c not in RECORD]
    assert not missing, (len(missing), missing[:5])
    assert set(RECORD) == set(cases)
    refused = [c for c, v in RECORD.items() if v == "refused"]
    ran = [c for c, v in RECORD.items() if v == "ok"]
    assert len(refused) == sweep.EXPECTED_REFUSALS
    assert len(ran) == len(cases) - sweep.EXPECTED_REFUSALS
    t = sweep.table()
    assert all(c[0] == "records" and t[c] != 0 for c in refused)
    seen = collections.defaultdict(set)
    for rows in INFOS.values():
        for _, tup in rows:
            for f, v in zip(INFO_FIELDS, tup):
                seen[f].add(v)
    want = dict(fwd_layout={0, 1, 2, 3, 4}, fwd_fixed={0, 1}, bwd_algo={1, 3}, fwd_waves={4, 8},
                fwd_unroll={4, 8}, bwd_waves={8, 12, 16}, bwd_unroll={8, 12})
    for f, values in want.items():
        assert values <= seen[f], (f, sorted(seen[f]))
    print(f"\nsweep: {len(ran)} cases ran, {len(refused)} documented refusals; seconds per "
          f"section: " + ", ".join(f"{s} {v:.1f}" for s, v in SECONDS.items()) +
          f"; total {sum(SECONDS.values()):.1f}")
    print("plan_info " + str(INFO_FIELDS))
    for (gname, oid), rows in INFOS.items():
        by = collections.defaultdict(list)
        for k, tup in rows:
            by[tup].append(k)
        for tup, ks in sorted(by.items(), key=lambda kv: min(kv[1])):
            print(f"  {gname} {oid}: {tup} k={k_ranges(ks)}")
